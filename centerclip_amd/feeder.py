"""Host -> device staging for the retrieval forward: the step the kernels are timed on takes batches that are already in
HBM; a loader hands over pinned host tensors.  ``DeviceFeeder`` keeps ``depth`` device-resident copies of a batch and fills
them on a COPY STREAM while the encoders work on the previous batch, so that the resident-input rate is reachable from a
loader: with the decoder's uint8 frames (N3: 1.8 MB per 12-frame clip, the normalisation runs inside the patch gather) a
16-clip batch is 29 MB = ~0.5 ms of PCIe Gen5 under 2.1 ms of compute.

    feeder = DeviceFeeder(device, depth=2)
    for slot, (ids, mask, video_u8, vmask) in feeder(loader):      # tensors of slot `slot`, valid until the next iteration
        out = model(ids, seg, mask, video_u8, vmask)                # (a hipGraph per slot works: the addresses are stable)

Ordering: the compute stream waits for the slot's copy event before it reads the slot; the copy stream waits for the
event the compute stream records when it is done with the slot before it overwrites it.  No host synchronisation.
PyTorch streams / events / ``Tensor.copy_(non_blocking=True)`` only: plumbing, no kernels of its own.

``frame_transform`` (a ``preprocess.FrameTransform``) takes decoded frames of any size: the loader hands over the raw uint8
video, the resize + centre crop runs on the copy stream right behind the slot's copy, into a second buffer of the slot, and that
buffer is yielded in the raw video's place - the consumer sees model-resolution frames at addresses that never change.
``video_index``: the video's position in the loader's tuple (default: its only 4-D / 6-D uint8 tensor).

A ragged batch (``preprocess.PackedClips`` in the video's place, ``frame_transform=preprocess.ClipCollate(...)``): the slot's
raw buffer is a byte buffer that grows geometrically and never shrinks - batches differ in their total bytes - filled by one
copy; the collate runs on the copy stream into the slot's fixed [B, 1, T, ...] cooked buffer, whose address never changes: that
is the address consumers and captured graphs see.  A batch of another B (or layout) gets new buffers, as a tensor batch of
another shape does.
"""
import torch

from .preprocess import PackedClips


def _fits(d, h):
    """whether slot entry d can take host entry h as it is"""
    if isinstance(h, PackedClips):
        return isinstance(d, PackedClips) and len(d) == len(h) and d.chw == h.chw
    return isinstance(d, torch.Tensor) and tuple(d.shape) == tuple(h.shape) and d.dtype == h.dtype


class DeviceFeeder:
    def __init__(self, device, depth=2, frame_transform=None, video_index=None):
        assert depth >= 2, "double buffering needs two slots"
        self.frame_transform, self.video_index = frame_transform, video_index
        self.cooked = [None] * depth                                 # per slot: the transform's output buffer, or None
        self.device = torch.device(device)
        self.depth = depth
        self.copy_stream = torch.cuda.Stream(self.device)
        self.slots = [None] * depth
        self.raw = [None] * depth                                    # per slot: the byte buffer of a PackedClips entry
        self.ready = [torch.cuda.Event() for _ in range(depth)]      # slot filled
        self.free = [torch.cuda.Event() for _ in range(depth)]       # slot no longer read by the compute stream
        self._used = [False] * depth

    def _fill(self, k, host_batch):
        host_batch = tuple(host_batch)
        if self.slots[k] is None or len(self.slots[k]) != len(host_batch) or not all(map(_fits, self.slots[k], host_batch)):
            # (a PackedClips entry: the table only - its bytes are pointed at the slot's byte buffer below, per batch)
            self.slots[k] = tuple(PackedClips(None, h.table, h.chw) if isinstance(h, PackedClips)
                                  else torch.empty(h.shape, dtype=h.dtype, device=self.device) for h in host_batch)
            self.cooked[k] = None
            if self.frame_transform is not None:
                video = host_batch[self._video_index(host_batch)]
                packed = isinstance(video, PackedClips)
                if not self.frame_transform.passes_through(video if packed else video.shape):
                    self.cooked[k] = torch.empty(self.frame_transform.output_shape(video if packed else video.shape),
                                                 dtype=torch.uint8, device=self.device)
            if any(isinstance(h, PackedClips) for h in host_batch) and self.cooked[k] is None:
                raise ValueError("DeviceFeeder: a PackedClips batch needs frame_transform=preprocess.ClipCollate(...)")
        with torch.cuda.stream(self.copy_stream):
            if self._used[k]:
                self.copy_stream.wait_event(self.free[k])
            else:
                # a freshly allocated slot may be memory the caching allocator took back from the compute stream with that
                # stream's last kernels on it still queued: the first copy into it waits for what is enqueued there
                self.copy_stream.wait_stream(torch.cuda.current_stream(self.device))
            for d, h in zip(self.slots[k], host_batch):
                if isinstance(h, PackedClips):
                    # the byte buffer is allocated and only ever used on the copy stream (the consumer sees the cooked buffer)
                    n = h.data.numel()
                    if self.raw[k] is None or self.raw[k].numel() < n:
                        self.raw[k] = torch.empty(max(n, 2 * self.raw[k].numel() if self.raw[k] is not None else 0),
                                                  dtype=torch.uint8, device=self.device)
                    d.data, d.table = self.raw[k][:n], h.table
                    d.data.copy_(h.data, non_blocking=True)
                else:
                    d.copy_(h, non_blocking=True)                    # asynchronous only from pinned memory
            if self.cooked[k] is not None:
                self.frame_transform(self.slots[k][self._video_index(host_batch)], out=self.cooked[k])
            self.ready[k].record(self.copy_stream)

    def _video_index(self, batch):
        if self.video_index is not None:
            return self.video_index
        dims = getattr(self.frame_transform, "frame_dims", (4, 6))          # (a YUV transform's frames are [..., 3H/2, W])
        dtypes = getattr(self.frame_transform, "frame_dtypes", (torch.uint8,))  # (16-bit YUV layouts: uint16 / int16 words)
        found = [i for i, t in enumerate(batch) if isinstance(t, PackedClips) or (t.dtype in dtypes and t.dim() in dims)]
        if len(found) != 1:
            raise ValueError("DeviceFeeder(frame_transform=...): the batch has %d frame tensors of the transform's dtype - pass video_index"
                             % len(found))
        return found[0]

    def _view(self, k):
        if self.cooked[k] is None:
            return self.slots[k]
        vi = self._video_index(self.slots[k])
        return self.slots[k][:vi] + (self.cooked[k],) + self.slots[k][vi + 1:]

    def __call__(self, host_batches):
        """Iterate over (slot index, device tensors) for an iterable of host batches (tuples of CPU tensors, ideally pinned)."""
        it = iter(host_batches)
        filled = []
        for k in range(self.depth):                                  # prime every slot
            try:
                self._fill(k, next(it))
                filled.append(k)
            except StopIteration:
                break
        while filled:
            k = filled.pop(0)
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(self.ready[k])
            yield k, (self.slots[k] if self.frame_transform is None else self._view(k))
            self.free[k].record(cur)                                 # everything the consumer enqueued on `cur` so far
            self._used[k] = True
            try:
                self._fill(k, next(it))
                filled.append(k)
            except StopIteration:
                pass
