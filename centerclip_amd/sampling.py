"""Which frames of a decoded video become a clip: the host-side index helpers of the reference's loaders
(dataloaders/sampling.py), in NumPy.  They run BEFORE the copy to the device - only the sampled frames are packed
(``preprocess.pack_clips``), or the whole video is packed and the index handed to ``preprocess.ClipCollate``:

    idx = uniform_sampling(T, len(video))                 # T offsets into the video, first frame = 0
    packed = pack_clips([video[idx], ...])                # or pack whole videos: ClipCollate(...)(packed, index=[idx, ...])

Mask rule (dataloaders/decode.py): a video shorter than the clip repeats its last frame - the offsets below are clipped to the
last frame - and the loader's video mask covers ``lengths = min(num_frames, clip_length)`` slots
(``PackedClips.video_mask(T, lengths=...)``).

``clip_length``: frames wanted; ``num_frames``: frames the video has; ``data_length``: consecutive frames taken per offset (the
last offset leaves room for them).  With ``rng=None`` the random draws are the reference's calls on the global
``numpy.random`` in the reference's order, so ``numpy.random.seed(s)`` reproduces its indices; any object with ``randint(high,
size=)`` and ``choice(n, k, replace=)`` (a ``numpy.random.RandomState``) can be passed instead.
"""
import numpy as np


def _consecutive(clip_length, num_frames, data_length):
    """Too few frames to spread over: 0, d, 2 d, ... clipped to the last offset that still has d frames behind it."""
    return np.clip(np.arange(0, clip_length * data_length, data_length), 0, num_frames - data_length)


def _centres(tick, clip_length):
    return [int(tick / 2.0 + tick * x) for x in range(clip_length)]


def uniform_sampling(clip_length, num_frames, data_length=1, twice_sample=False):
    """Evenly spaced offsets: the centres of ``clip_length`` equal segments of the video; ``twice_sample`` appends the segments'
    starts (2 * clip_length offsets).  A video with no more than clip_length + data_length - 1 frames: consecutive offsets,
    clipped to the last frame.  -> int array."""
    if num_frames > clip_length + data_length - 1:
        tick = (num_frames - data_length + 1) / float(clip_length)
        offsets = _centres(tick, clip_length)
        if twice_sample:
            offsets = offsets + [int(tick * x) for x in range(clip_length)]
        return np.array(offsets)
    return np.array(_consecutive(clip_length, num_frames, data_length))


def multi_segments_sampling(clip_length, num_frames, random_shift=True, data_length=1, rng=None):
    """TSN-style segment sampling.  ``random_shift=True`` (training): one random frame per segment - segment starts plus ONE
    ``randint(average_duration, size=clip_length)``; where the segments are shorter than one frame but the video still has more
    than clip_length frames, ONE sorted ``choice(num_frames, clip_length, replace=False)``; else consecutive offsets.
    ``random_shift=False``: the segments' centres, as ``uniform_sampling``.  -> int array [clip_length]."""
    rng = np.random if rng is None else rng
    if not random_shift:
        return uniform_sampling(clip_length, num_frames, data_length)
    average_duration = (num_frames - data_length + 1) // clip_length
    if average_duration > 0:
        return np.multiply(list(range(clip_length)), average_duration) + rng.randint(average_duration, size=clip_length)
    if num_frames > clip_length:
        return np.sort(rng.choice(num_frames, clip_length, replace=False))
    return _consecutive(clip_length, num_frames, data_length)


__all__ = ["uniform_sampling", "multi_segments_sampling"]
