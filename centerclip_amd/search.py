"""Retrieval over a cached gallery (not in the reference, whose only consumer of the cached features is the [Nt, Nv] matrix
of eval_epoch): ``FeatureGallery`` keeps the similarity operands of the clips (or captions) added to it on the device and
answers "the k best and their scores" for a batch of queries with ``torch.ops.centerclip.similarity_topk`` - one pass over
the gallery rows, no [Nq, N] matrix, memory that does not grow with the gallery.

    gallery = FeatureGallery(model)                       # side="video": clips in, captions as queries
    pos = gallery.add(video, video_mask)                  # any number of batches
    scores, ids = gallery.search(input_ids, k=10)         # [Nq, 10] fp32, [Nq, 10] int64 positions

The rows are what eval_epoch caches (``eval._video_operand`` / ``HipBackend.text_operand``: split-fp16 planes, [n, 3E]), the
scores are the bits of eval_epoch's matrix for the same pair, and the order is the stable descending sort of its row (equal
scores by smaller position).  ``similarity`` gives that matrix itself for small galleries and for checking.

``dual_softmax=True`` ranks the CAMoE dual softmax D = S * softmax(S, dim=0) * Nt of ``eval_epoch(camoe_dsl=1)`` instead of S,
still without the matrix: D[i, j] needs two floats per video j - the maximum and the exp-sum of column j over the captions -
which ``torch.ops.centerclip.dsl_col_stats_planes`` takes from the operand rows and ``similarity_topk_dsl`` applies.

    gallery = FeatureGallery(model, dual_softmax=True)    # clips in; the captions the softmax runs over are a bank
    gallery.set_query_bank(all_input_ids)                 # before or after the clips: the same bits
    gallery.add(video, video_mask)
    scores, ids = gallery.search(input_ids, k=10)         # rows of eval_epoch's text->video D for captions of the bank

``grouped=True`` ranks GROUPS of adjacent rows, each by its best row - the sentences of a video (the multi-sentence sets:
eval_epoch ranks video->text on the maximum over a video's sentences) or the windows of a long video - with
``similarity_topk_grouped`` (``_dsl``): still one pass, no matrix, exact.

    gallery = FeatureGallery(model, side="text", grouped=True)
    gallery.add(input_ids, group=video_index)             # one label for the batch, or one per row; equal neighbours = a group
    scores, groups, pos = gallery.search_groups(video, video_mask, k=10)    # the 10 best videos, each by its best sentence

Rows leave and searches narrow with one bit per row (``similarity_topk_masked``), without re-encoding or a second gallery:

    gallery.remove(pos[:3])                               # no longer ranked; the other rows keep their positions
    tenant = gallery.row_mask(positions=mine)             # built once on the host ...
    scores, ids = gallery.search(input_ids, k=10, allow=tenant)             # ... passed to any number of searches
    new_pos = gallery.compact()                           # drop the holes: the gallery of the surviving rows

"Where does THIS row stand for THIS query" - the rank R@k, MdR and MnR are made of - comes from the same stream
(``similarity_rank``): counts against the target's own score instead of a list, so any place, not only the first 128:

    ranks, scores, counts = gallery.rank(input_ids, target=truth)           # 0-based places in search's full ordering
    ranks, scores, counts = gallery.rank_groups(video, video_mask, target=labels)      # grouped=True: the place of a group

Lists of up to 4096 entries and "next page" cursors (``similarity_topk_deep``): pages of at most 128, each the same stream
restricted to what lies behind the page before - exact, no matrix, no state between calls.  The gallery asks this one op
for every list; up to 128 entries without a cursor it is one page, the launches of the ops named above:

    scores, ids = gallery.search(input_ids, k=1000)                         # candidates for a re-ranker
    more_scores, more_ids = gallery.search(input_ids, k=50, after=(scores[:, -1], ids[:, -1]))     # entries 1000..1049

"Which video, and where in it": a long video is encoded once and every sliding window of it becomes a row
(``video_window_pool_planes``: the pooling of ``add`` on the window's segments, one launch for all windows), a video one group:

    gallery = FeatureGallery(model, grouped=True)
    pos, windows = gallery.add_windows(video, lengths, window=[8, 16], group=video_ids)     # video [b, 1, F, ...], F = n * T frames
    scores, videos, best = gallery.search_groups(input_ids, k=10)
    frames = gallery.windows(best[0].cpu())                                 # (start_frame, stop_frame) of each best window
"""
import numpy as np
import torch

from . import _lib as L
from . import torch_ops as T
from .cluster.shift import SHIFT_ALGORITHMS
from .eval import HipBackend, _video_operand

SIDES = ("video", "text")


def _host_ints(value, what, name):
    """The one reading of a host integer argument: an int, a flat host sequence of ints or a CPU LongTensor (0-D or 1-D) ->
    int64 array [n].  Anything else is the one ValueError - a device tensor above all: it would have to be read, and reading
    synchronises.  ``what``: the method, for the message ("FeatureGallery.rank_groups"); ``name``: what the values are
    called ("labels")."""
    arr = None
    if torch.is_tensor(value):
        if value.device.type == "cpu" and value.dtype == torch.int64 and value.dim() <= 1:
            arr = value.numpy().reshape(-1)
    elif isinstance(value, (int, np.integer)):
        arr = np.array([int(value)])
    else:
        try:
            arr = np.asarray(list(value))
        except (TypeError, ValueError):                          # (not iterable; a ragged nest)
            pass
    if arr is None or arr.ndim != 1 or (arr.size and arr.dtype.kind not in "iu"):
        got = "a %s %s tensor %s" % (value.device, value.dtype, tuple(value.shape)) if torch.is_tensor(value) else "%.60r" % (value,)
        raise ValueError("%s: %s are an int, a flat host sequence of ints or a CPU LongTensor, not %s (reading a device "
                         "tensor would synchronise)" % (what, name, got))
    return arr.astype(np.int64)


def _exactly(arr, n, what, name, per):
    if arr.size != n:
        raise ValueError("%s: %d %s, not one per %s (%d)" % (what, arr.size, name, per, n))
    return arr


def _scales(value, frame_duration, what, count=None):
    """an int, or one int per scale -> list of segment counts; every value a positive multiple of frame_duration"""
    if isinstance(value, (int, np.integer)):
        values = [value] * (count or 1)
    elif isinstance(value, (list, tuple, np.ndarray)):
        values = list(value)
    else:
        raise ValueError("window_table: %s is an int or a sequence of ints, not %r" % (what, value))
    if not values or (count is not None and len(values) != count):
        raise ValueError("window_table: %s holds %d values for %s scales" % (what, len(values), count if count is not None else "no"))
    for v in values:
        if not isinstance(v, (int, np.integer)) or v <= 0 or v % frame_duration:
            raise ValueError("window_table: %s %r is not a positive multiple of the %d frames of a segment"
                             % (what, v, frame_duration))
    return [int(v) // frame_duration for v in values]


def window_table(lengths, frame_duration, window, stride=None, segments=None):
    """The sliding windows of long videos, in segments: -> np.int64 [nW, 3], columns (video, start_seg, stop_seg).  Pure host
    work.  ``lengths``: the valid frames of every video (a host sequence or a CPU LongTensor - never a device tensor: reading
    it would synchronise); video i has n_i = lengths[i] // frame_duration valid segments (a segment is valid when its last
    frame is - ``get_video_mask_after_cluster`` - so a partial last segment is dropped); none at all, or more than
    ``segments`` (when given): ValueError.  ``window``: frames per window, an int or one per scale; ``stride``: an int for all
    scales or one per scale, default half the window rounded down to whole segments (at least one); all positive multiples
    of ``frame_duration``.  Per video and scale: n_i <= w gives the one window (0, n_i); otherwise the starts 0, s, 2s, ...
    <= n_i - w, and one more at n_i - w when the last is not there, so every valid segment is covered.  Order: video, scale
    as given, start; inside a video a (start, stop) pair appears once (the first stays)."""
    fd = int(frame_duration)
    if fd <= 0:
        raise ValueError("window_table: frame_duration %d" % fd)
    lens = _host_ints(lengths, "window_table", "lengths")
    ws = _scales(window, fd, "window")
    if stride is None:
        ss = [max(w // 2, 1) for w in ws]
    else:
        ss = _scales(stride, fd, "stride", len(ws))
    rows = []
    for i, length in enumerate(lens.tolist()):
        n = int(length) // fd
        if n <= 0:
            raise ValueError("window_table: video %d has %d frames, not one whole segment of %d" % (i, length, fd))
        if segments is not None and n > int(segments):
            raise ValueError("window_table: video %d has %d valid segments, the features hold %d" % (i, n, int(segments)))
        seen = set()
        for w, s in zip(ws, ss):
            if n <= w:
                spans = [(0, n)]
            else:
                starts = list(range(0, n - w + 1, s))
                if starts[-1] != n - w:
                    starts.append(n - w)
                spans = [(a, a + w) for a in starts]
            for span in spans:
                if span not in seen:
                    seen.add(span)
                    rows.append((i,) + span)
    return np.array(rows, dtype=np.int64).reshape(-1, 3)


class FeatureGallery:
    """``side``: what the gallery holds - "video" (queries are captions) or "text" (queries are clips).  ``capacity``: rows
    to allocate up front; the buffer grows geometrically and keeps its rows bit for bit.  ``products``: the fp16 products per
    multiply-add of a score (``HipBackend.with_products``); None = ``HipBackend.similarity_products``.  The scores are
    exp(logit_scale) * cosine as in ``eval._similarity_matrix``; a ``camoe_dsl`` model is refused unless
    ``dual_softmax=True``: the dual softmax needs column statistics over all queries and is no per-query ranking.

    ``dual_softmax=True`` (whatever the model's flag): ``search*`` and ``similarity*`` rank
    D[t, v] = n_total * S[t, v] * exp(S[t, v] - m_v) / s_v, with (m_v, s_v) the maximum and the exp-sum of S[:, v] over a set
    of captions, in the fp32 operations of ``dsl_apply_``.
      * side="video": that set is the bank registered with ``set_query_bank`` / ``set_query_bank_features`` (its operand rows
        stay on the device; n_total = its size).  The pair of every clip held is computed when the bank is set and of every
        clip added later when it is added - the same bits either way, whatever the batches.  With the bank equal to the
        evaluation captions and a query that is one of them, the scores are a row of the matrix ``eval_epoch(camoe_dsl=1)``
        ranks text->video; for any other query they are the same formula with the bank's statistics, the query not
        included.  Searching without a bank raises ValueError.  The pairs are taken with the model's logit scale at that
        moment: set the bank again after changing it.
      * side="text": no bank (``set_query_bank*`` raises ValueError).  Every search first takes the query clips' pairs over the
        captions held (n_total = len(self)), then the top-k: two passes over the gallery.  With the gallery holding all
        evaluation captions of a set with ONE caption per video this is a row of ``eval_epoch``'s video->text ranking (D^T).
        On the multi-sentence sets (MSVD, ActivityNet, DiDeMo) eval_epoch ranks the maximum over a video's sentences:
        that is ``search_groups`` of a ``grouped=True`` gallery whose labels are the videos, not ``search``.

    ``grouped=True``: every row carries an int64 label (``add(..., group=)``); adjacent rows with equal labels form a group,
    which may continue across ``add`` calls but not return after another label.  ``search_groups*`` -> (scores, labels,
    positions) of the k best groups, each by its best row: of ``search``'s row order the first k rows that are the first of
    their group to appear (equal scores: the smaller position, between groups and inside one); (-inf, -1, -1) beyond the
    number of groups.  ``search*`` keep ranking rows.  With dual_softmax=True the statistics are what they are without
    groups - side="text": over all captions held - so the group maximum of D is what eval_epoch ranks video->text on the
    multi-sentence sets.

    Removing and restricting (``similarity_topk_masked``: a bit per row, still one pass, exact): ``remove(positions)`` /
    ``remove_groups(labels)`` take rows out - the others keep their positions, ``len(gallery)`` counts the rows held,
    ``gallery.span`` the positions in use, ``compact()`` closes the holes and returns the map old -> new position.
    ``search*(..., allow=mask)`` ranks a subset (``row_mask`` builds one on the host).  The ranking sees ``allow & live``; the
    results are those of a gallery holding only these rows, at their positions here.  dual_softmax=True: side="video" - a
    clip's statistics never depended on other clips; side="text" - the statistics run over the captions still held
    (n_total = len(self)), and ``allow`` restricts the ranking, not the softmax.  A gallery that never removes a row and
    never gets ``allow=`` allocates and launches what it did without any of this.

    The rank of a known row or group (``similarity_rank``: three launches, no matrix, no list, exact): ``rank*(..., target=)``
    -> (ranks, scores, counts) of one target position per query among the rows ``search*`` ranks - removals, ``allow=`` and
    the dual softmax's statistics act as there; ``rank_groups*`` the same for one target label per query among the groups
    ``search_groups*`` ranks.  ``counts`` are the (greater, equal, equal in front) triples of ``rank_counts_cols`` on the
    matrix row, ``ranks = counts[:, 0] + counts[:, 2]``; a target that is not selectable keeps its score and is not counted.

    The contract of a list, for every ``search*`` method and every combination above, 1 <= k <= 4096:
      * ``search(k=K)`` is the first K entries of the stable descending sort of ``similarity()``'s row: the scores are the
        matrix op's bits, equal scores are ordered by smaller position, (-inf, -1) fills what lies behind the selectable rows
        (``search_groups``: of that order the first row of every group).
      * ``search(k=a)`` followed by ``search(k=b, after=(scores[:, -1], positions[:, -1]))`` of its result is columns
        [a, a + b) of ``search(k=a + b)``.  A cursor is nothing but that pair: it names a place in the ordering, not a row that
        must still be held, so it stays right when rows are removed between the two calls (the list continues behind the
        place the pair had); a cursor equal to the fill gives the fill.  ``compact()`` renumbers positions: cursors do not
        survive it.
      * Every list is ``similarity_topk_deep``: ceil(k / 128) passes over the gallery (pages of 127 at E = 1024 with three
        products, so k = 128 there takes two), the pages handing over on the device - k <= 128 without ``after=`` is one pass,
        the launches of the specialised ops; dual_softmax=True, side="text": the queries' statistics are taken once per
        call, not per page.
      * A call does not synchronise with the host: ``after=`` takes device tensors and reads none of them."""

    def __init__(self, model, side="video", capacity=0, products=None, dual_softmax=False, grouped=False):
        if side not in SIDES:
            raise ValueError("FeatureGallery: side is 'video' or 'text', not %r" % (side,))
        core = model.module if hasattr(model, 'module') else model
        if getattr(core, "camoe_dsl", False) and not dual_softmax:
            raise ValueError("FeatureGallery: camoe_dsl ranks S * softmax(S, dim=0) * Nt, which depends on every query at once "
                             "(dual_softmax=True ranks it against a registered set of captions)")
        products = HipBackend.similarity_products if products is None else int(products)
        self.backend = HipBackend.with_products(products)        # (raises for anything but 1, 2, 3)
        self.device = next(core.parameters()).device
        if self.device.type != "cuda":
            raise L.CenterClipHipError("FeatureGallery runs on MI355X only: the model is on %s (no CPU fallback)" % self.device)
        self.model, self.core, self.side, self.products = model, core, side, products
        self.E = int(core.clip_config['embed_dim'])
        self._rows = torch.zeros((max(int(capacity), 0), 3 * self.E), device=self.device, dtype=torch.float16)
        self._n = 0
        self.dual_softmax = bool(dual_softmax)
        if self.dual_softmax:
            self._bank = None                                    # side="video": operand rows of the captions, [n_bank, 3E]
            self._m = torch.zeros(self._rows.shape[0], device=self.device)       # per row held (side="video"): max_t S[t, v]
            self._s = torch.zeros(self._rows.shape[0], device=self.device)       # and sum_t exp(S[t, v] - m_v) over the bank
        self._forget_removals()                                  # (nothing is allocated until the first remove)
        self._win_host = None                                    # (nor until the first window row: _window_records)
        self.grouped = bool(grouped)
        if self.grouped:
            self._head = torch.zeros(self._rows.shape[0], device=self.device, dtype=torch.int32)     # first row of the row's group
            # mirror of the labels, one entry longer than the rows: the last one stays -1, which is what position -1 (the
            # fill) reads - the gather of a result's labels is one indexing launch
            self._label_dev = torch.full((self._rows.shape[0] + 1,), -1, device=self.device, dtype=torch.int64)
            self._reset_groups()

    def __len__(self):
        """Rows held: the positions in use minus the removed ones."""
        return self._n if self._live is None else int(self._live_count)

    @property
    def span(self):
        """Positions in use, removed ones included: the next row added gets position ``span``."""
        return self._n

    def clear(self):
        """Empty the rows and the groups and forget the removals (a dual-softmax gallery keeps its bank)."""
        self._n = 0
        self._forget_removals()
        self._win_host = None
        if self._grouped:
            self._reset_groups()

    @property
    def _dsl(self):
        return getattr(self, "dual_softmax", False)                # (an instance built without the constructor: plain)

    @property
    def _grouped(self):
        return getattr(self, "grouped", False)

    @property
    def _live(self):
        """None until the first ``remove``; then a NumPy bool per position in use, False = removed (the host mirror of
        the device words ``_live_dev``)"""
        return getattr(self, "_live_host", None)               # (an instance built without the constructor: nothing removed)

    @property
    def num_groups(self):
        """Groups held (grouped=True); after ``remove``: the groups with a row still held."""
        self._need_grouped("num_groups")
        if self._live is None:
            return self._groups
        return int(np.unique(self.labels.numpy()[self._live]).size)      # (a label never returns: one label, one group)

    @property
    def labels(self):
        """The label of every position in use, a CPU LongTensor [span] (grouped=True); removed rows keep theirs until
        ``compact()``."""
        self._need_grouped("labels")
        if len(self._label_chunks) != 1:
            self._label_chunks = [torch.cat(self._label_chunks) if self._label_chunks else torch.zeros(0, dtype=torch.int64)]
        return self._label_chunks[0]

    @property
    def rows(self):
        """The operand rows of the positions in use, [span, 3E] fp16 (a view of the buffer; removed rows included until
        ``compact()``)."""
        return self._rows[:self._n]

    # ------------------------------------------------------------------ operand rows of either side
    def _encode(self, **inputs):
        L.require_device(*inputs.values())
        was_training = self.model.training
        self.model.eval()
        try:
            with torch.no_grad():
                return self.model(**inputs)
        finally:
            self.model.train(was_training)

    def _video_rows(self, visual_output, video_mask):
        L.require_device(visual_output, video_mask)
        if visual_output.dim() != 2 and video_mask is None:
            raise ValueError("FeatureGallery: per-segment visual features need their video_mask")
        with torch.no_grad():
            return _video_operand(self.core, visual_output, video_mask, self.backend)

    def _text_rows(self, sequence_output):
        L.require_device(sequence_output)
        with torch.no_grad():
            return self.backend.text_operand(sequence_output.reshape(sequence_output.shape[0], -1))

    def _encode_video(self, video, video_mask):
        return self._video_rows(self._encode(video=video, video_mask=video_mask)['visual_output'], video_mask)

    def _encode_text(self, input_ids):
        return self._text_rows(self._encode(input_ids=input_ids)['sequence_output'])

    # ------------------------------------------------------------------ filling
    def _append(self, rows, group=None):
        if rows.dim() != 2 or rows.shape[1] != 3 * self.E:
            raise ValueError("FeatureGallery: operand rows of width %d, the model's embed_dim gives %d"
                             % (rows.shape[-1], 3 * self.E))
        start, n = self._n, self._n + rows.shape[0]
        plan = self._plan_groups(group, start, rows.shape[0]) if self._grouped else None     # (raises before anything is written)
        if n > self._rows.shape[0]:
            grown = torch.zeros((max(n, 2 * self._rows.shape[0]), 3 * self.E), device=self.device, dtype=torch.float16)
            grown[:start] = self._rows[:start]
            self._rows = grown
            for name in (("_m", "_s") if self._dsl else ()) + (("_head",) if self._grouped else ()):
                old = getattr(self, name)
                new = torch.zeros(grown.shape[0], device=self.device, dtype=old.dtype)
                new[:start] = old[:start]
                setattr(self, name, new)
            if self._grouped:
                labels = torch.full((grown.shape[0] + 1,), -1, device=self.device, dtype=torch.int64)
                labels[:start] = self._label_dev[:start]
                self._label_dev = labels
        self._rows[start:n] = rows
        self._n = n
        if self._live is not None and n > start:                 # rows behind removed ones: new positions, live
            self._live_host = np.concatenate((self._live, np.ones(n - start, dtype=bool)))
            self._live_count += n - start
            self._upload_live(start >> 5, T.mask_words(n))
        if plan is not None:
            self._take_groups(plan, start, n)
        if self._dsl:
            self._take_stats(start, n)
        return torch.arange(start, n)

    # ------------------------------------------------------------------ dual softmax: the bank and the rows' statistics
    def _take_stats(self, start, stop):
        """(m, s) of the clips [start, stop) over the bank (side="video" with a bank; otherwise nothing to do)"""
        if self.side != "video" or self._bank is None or stop <= start:
            return
        m, s = torch.ops.centerclip.dsl_col_stats_planes(self._bank, self._rows[start:stop], self._bank.shape[0], stop - start,
                                                         self._mult(), self.products)
        self._m[start:stop], self._s[start:stop] = m, s

    def _set_bank(self, encode, source):
        if not self._dsl or self.side != "video":
            raise ValueError("FeatureGallery.set_query_bank: only a dual_softmax=True gallery of side 'video' has a bank")
        self._bank = encode(source).clone()
        self._take_stats(0, self._n)

    def set_query_bank(self, input_ids):
        """Register the captions the dual softmax runs over (side="video", dual_softmax=True): encode them as ``search`` does,
        keep their operand rows and take the statistics of every clip held.  Replacing the bank recomputes them all."""
        self._set_bank(self._encode_text, input_ids)

    def set_query_bank_features(self, sequence_output):
        """``set_query_bank`` for captions encoded elsewhere (their sequence_output)."""
        self._set_bank(self._text_rows, sequence_output)

    def _query_stats(self, q):
        """side="text": the query clips' (m, s) over the captions held (after ``remove``: over those still held, whatever a
        search's ``allow=`` says - it restricts the ranking, not the softmax)"""
        if self._live is not None:
            return torch.ops.centerclip.dsl_col_stats_planes_masked(self._rows, q, self._n, q.shape[0], self._mult(),
                                                                    self.products, self._live_words())
        return torch.ops.centerclip.dsl_col_stats_planes(self._rows, q, self._n, q.shape[0], self._mult(), self.products)

    def _need_bank(self):
        if self.side == "video" and self._bank is None:
            raise ValueError("FeatureGallery: dual_softmax=True needs the captions the softmax runs over: set_query_bank first")

    # ------------------------------------------------------------------ groups (grouped=True): the labels' bookkeeping, on the host
    def _need_grouped(self, what):
        if not self._grouped:
            raise ValueError("FeatureGallery.%s: only a grouped=True gallery has groups" % what)

    def _reset_groups(self):
        self._label_chunks = []                                  # CPU LongTensors: the label of every row held
        self._closed = set()                                     # labels of the groups that ended: they must not return
        self._open = None                                        # (label, first row) of the last group: it may continue
        self._groups = 0

    def _check_group_arg(self, group, what):
        """the refusals that need nothing encoded: a grouped gallery wants ``group=``, a plain one refuses it"""
        if self._grouped and group is None:
            raise ValueError("FeatureGallery.%s: a grouped=True gallery needs group= (one label, or one per row)" % what)
        if not self._grouped and group is not None:
            raise ValueError("FeatureGallery.%s: group= needs a grouped=True gallery" % what)
        if torch.is_tensor(group) and (group.device.type != "cpu" or group.dtype != torch.int64):
            raise ValueError("FeatureGallery.%s: group labels are an int, a host sequence or a CPU LongTensor, not a %s %s "
                             "tensor (reading a device tensor would synchronise)" % (what, group.device, group.dtype))

    def _plan_groups(self, group, start, b):
        """The labels of the b rows about to get positions start.. -> (labels int64 [b], heads int32 [b], runs): checks only,
        no state is changed.  A label that returns after another one came in between: ValueError."""
        self._check_group_arg(group, "add")
        if isinstance(group, (int, np.integer)):
            lab = np.full(b, int(group), dtype=np.int64)
        else:
            lab = np.ascontiguousarray(group.numpy() if torch.is_tensor(group) else np.asarray(list(group)))
            if lab.shape != (b,) or (b and lab.dtype.kind not in "iu"):
                raise ValueError("FeatureGallery: group= holds %s labels of kind %r for %d rows (one int, or one int per row)"
                                 % (lab.shape, lab.dtype.kind, b))
            lab = lab.astype(np.int64)
        if b == 0:
            return lab, np.zeros(0, dtype=np.int32), []
        first = np.flatnonzero(np.concatenate(([True], lab[1:] != lab[:-1])))         # where a run of equal labels starts
        runs = [int(v) for v in lab[first]]
        continues = self._open is not None and runs[0] == self._open[0]
        new = runs[1:] if continues else runs
        back = [v for v in new if v in self._closed or (self._open is not None and v == self._open[0])]
        if back or len(set(new)) != len(new):
            raise ValueError("FeatureGallery: group label %s returns after another label came in between (the rows of a group "
                             "are adjacent)" % (back[0] if back else [v for v in new if new.count(v) > 1][0]))
        head_of_run = start + first
        if continues:
            head_of_run[0] = self._open[1]
        heads = np.repeat(head_of_run, np.diff(np.concatenate((first, [b])))).astype(np.int32)
        return lab, heads, (new, int(head_of_run[-1]))

    def _host_to_device(self, array):
        t = torch.from_numpy(array)
        if self.device.type != "cuda":
            return t
        return t.pin_memory().to(self.device, non_blocking=True)                       # (no synchronisation)

    def _take_groups(self, plan, start, n):
        lab, heads, runs = plan
        if n == start:
            return
        new, last_head = runs
        if new:
            if self._open is not None:
                self._closed.add(self._open[0])
            self._closed.update(new[:-1])
            self._open = (new[-1], last_head)
            self._groups += len(new)
        self._label_chunks.append(torch.from_numpy(lab.copy()))
        self._head[start:n] = self._host_to_device(heads)
        self._label_dev[start:n] = self._host_to_device(lab)

    def add(self, *inputs, group=None):
        """``add(video, video_mask)`` (``add(input_ids)`` for side="text"): encode a batch as eval_epoch does and append
        its rows -> the positions they got (LongTensor).  grouped=True: ``group=`` is the rows' label - an int for the whole
        batch, or a host sequence / CPU LongTensor with one label per row (never a device tensor: no synchronisation)."""
        self._check_group_arg(group, "add")
        return self._append(self._encode_video(*inputs) if self.side == "video" else self._encode_text(*inputs), group)

    def add_features(self, features, mask=None, group=None):
        """The same for features cached elsewhere: ``add_features(visual_output, video_mask)`` ([b, T', E] per-segment
        features with the loader's mask, or [b, E] pooled rows) or, side="text", ``add_features(sequence_output)``."""
        self._check_group_arg(group, "add_features")
        return self._append(self._video_rows(features, mask) if self.side == "video" else self._text_rows(features), group)

    # ------------------------------------------------------------------ windows of long videos
    def _window_records(self):
        """None until a window row exists; then int64 [span, 2] on the host: the (start_frame, stop_frame) every position
        stands for, (-1, -1) for the rows of ``add`` / ``add_features`` (padded here: those methods know nothing of it)"""
        rec = getattr(self, "_win_host", None)                   # (an instance built without the constructor: none)
        if rec is not None and rec.shape[0] < self._n:
            rec = self._win_host = np.concatenate((rec, np.full((self._n - rec.shape[0], 2), -1, dtype=np.int64)))
        return rec

    def _append_windows(self, rows, frames, group=None):
        """``_append`` for window rows: ``frames`` int64 [n, 2] = the (start_frame, stop_frame) of every row"""
        pos = self._append(rows, group)                          # (raises before anything is written)
        if frames.shape[0]:
            rec = self._window_records()
            head = rec[:self._n - frames.shape[0]] if rec is not None else np.full((self._n - frames.shape[0], 2), -1, dtype=np.int64)
            self._win_host = np.concatenate((head, frames.astype(np.int64)))
        return pos

    def windows(self, positions):
        """The frames the rows at ``positions`` (as ``remove`` takes them) stand for -> CPU LongTensor [n, 2] of
        (start_frame, stop_frame) inside their video; (-1, -1) for rows that came from ``add`` / ``add_features``.  Kept on the
        host like the labels: the records survive ``remove``, move with their rows in ``compact()``, go with ``clear()``."""
        pos = self._positions(positions, "windows")
        rec = self._window_records()
        return torch.from_numpy(rec[pos] if rec is not None else np.full((pos.size, 2), -1, dtype=np.int64))

    def _need_video_side(self, what):
        if self.side != "video":
            raise ValueError("FeatureGallery.%s: windows are rows of a side='video' gallery, not side=%r" % (what, self.side))

    def _window_groups(self, group, table, b, what):
        """``group=`` of a window call - an int, or one label per VIDEO - expanded to the rows of ``table``"""
        self._check_group_arg(group, what)
        if group is None or isinstance(group, (int, np.integer)):
            return group
        what = "FeatureGallery." + what
        return _exactly(_host_ints(group, what, "group= labels"), b, what, "group= labels", "video")[table[:, 0]]

    def _window_rows(self, visual_output, table):
        """per-segment features [b, S, E] + the segment table -> the windows' operand rows [nW, 3E]"""
        visual = visual_output.float().contiguous()
        if getattr(self.core, "sim_header", "meanP") != "seqTransf":
            return torch.ops.centerclip.video_window_pool_planes(visual, self._host_to_device(table.astype(np.int32)))
        # seqTransf: the head is part of a clip's operand and its position rows start at 0 for every clip - the windows of
        # one length are gathered and go through the head as a batch of clips (the longest first: a window beyond the
        # position table raises the head's own ValueError before any row exists)
        rows = torch.empty((table.shape[0], 3 * self.E), device=self.device, dtype=torch.float16)
        span = table[:, 2] - table[:, 1]
        for n in sorted(set(span.tolist()), reverse=True):
            which = np.flatnonzero(span == n)
            seg = (table[which, 0] * visual.shape[1] + table[which, 1])[:, None] + np.arange(n)[None, :]
            clips = visual.view(-1, visual.shape[2])[self._host_to_device(seg.reshape(-1))].view(which.size, n, -1)
            ones = torch.ones((which.size, n), device=self.device, dtype=torch.long)
            rows[self._host_to_device(which)] = self._video_rows(clips, ones)
        return rows

    def _add_window_features(self, visual_output, table, group):
        fd = int(self.core.f_frame_duration)
        frames = table * np.array([1, fd, fd], dtype=np.int64)
        with torch.no_grad():
            rows = self._window_rows(visual_output, table)
        return self._append_windows(rows, frames[:, 1:], group), torch.from_numpy(frames)

    def add_window_features(self, visual_output, lengths, window, stride=None, group=None):
        """The sliding windows of long videos from per-segment features encoded ONCE (side="video").  ``visual_output``
        [b, S, E]: the features of the b videos' segments, before any head; ``lengths``: the valid frames of every video (a
        host sequence or a CPU LongTensor); ``window`` / ``stride``: frames, as ``window_table`` takes them (a multiple of
        ``core.f_frame_duration``; several windows = several scales).  Every window becomes one row, the bits of
        ``add_features(visual_output[v:v+1, a:b], ones)`` for meanP (one launch for all of them:
        ``video_window_pool_planes``); seqTransf runs the head on every window as on a clip.  ``group=``: an int, or one label
        per VIDEO - all windows of a video form one group, so ``search_groups`` answers "which video" and the position it
        returns "where": ``windows(position)``.  -> (positions, windows): the rows' positions and a CPU LongTensor
        [n_rows, 3] of (video index in this call, start_frame, stop_frame)."""
        self._need_video_side("add_window_features")
        L.require_device(visual_output)
        if visual_output.dim() != 3 or visual_output.shape[2] != self.E:
            raise ValueError("FeatureGallery.add_window_features: per-segment features [b, S, %d], not %s"
                             % (self.E, tuple(visual_output.shape)))
        b, S = visual_output.shape[:2]
        lens = _host_ints(lengths, "FeatureGallery.add_window_features", "lengths")
        table = window_table(lens, int(self.core.f_frame_duration), window, stride, segments=S)
        if b == 0 or lens.size != b:
            raise ValueError("FeatureGallery.add_window_features: %d lengths for %d videos" % (lens.size, b))
        return self._add_window_features(visual_output, table, self._window_groups(group, table, b, "add_window_features"))

    def add_windows(self, video, lengths, window, stride=None, group=None, encode_batch=64):
        """The same from frames: ``video`` [b, 1, F, ...] as ``add`` takes it, F any positive multiple of the model's clip
        length T.  The frames are folded to b F / T clips of T frames and encoded as ``add`` encodes clips (at most
        ``encode_batch`` per call) - every frame once, whatever the windows - and their per-segment features, viewed as
        [b, F / fd, E], go through ``add_window_features``.  Refused, before anything is encoded: the shift algorithms
        and linear_patch='3d' (neighbouring frames mix, so a segment's feature is not its own frames' alone), F % T != 0,
        lengths[i] > F."""
        self._need_video_side("add_windows")
        core = self.core
        if getattr(core, "cluster_algo", None) in SHIFT_ALGORITHMS:
            raise ValueError("FeatureGallery.add_windows: cluster_algo=%r shifts channels between neighbouring frames, so a "
                             "segment's feature depends on the clip it was cut into" % core.cluster_algo)
        if getattr(core, "linear_patch", "2d") == "3d":
            raise ValueError("FeatureGallery.add_windows: linear_patch='3d' mixes neighbouring frames in the patch embedding, "
                             "so a segment's feature depends on the clip it was cut into")
        if getattr(core, "pre_visual_pooling", 0):
            raise ValueError("FeatureGallery.add_windows: pre_visual_pooling pools the clip inside the model; the windows need "
                             "the per-segment features")
        T, fd = int(core.video_frames), int(core.f_frame_duration)
        if video.dim() < 4 or video.shape[1] != 1:
            raise ValueError("FeatureGallery.add_windows: video is [b, 1, F, ...], not %s" % (tuple(video.shape),))
        b, F = int(video.shape[0]), int(video.shape[2])
        if F <= 0 or F % T:
            raise ValueError("FeatureGallery.add_windows: %d frames are not a positive multiple of the model's clip length %d"
                             % (F, T))
        if int(encode_batch) < 1:
            raise ValueError("FeatureGallery.add_windows: encode_batch %d" % int(encode_batch))
        lens = _host_ints(lengths, "FeatureGallery.add_windows", "lengths")
        table = window_table(lens, fd, window, stride)
        if b == 0 or lens.size != b:
            raise ValueError("FeatureGallery.add_windows: %d lengths for %d videos" % (lens.size, b))
        over = np.flatnonzero(lens > F)
        if over.size:
            raise ValueError("FeatureGallery.add_windows: video %d is longer than the %d frames given" % (int(over[0]), F))
        group = self._window_groups(group, table, b, "add_windows")
        L.require_device(video)
        clips = video.reshape((b * (F // T), 1, T) + tuple(video.shape[3:]))
        ones = torch.ones((min(int(encode_batch), clips.shape[0]), T), device=video.device, dtype=torch.long)
        parts = []
        for c0 in range(0, clips.shape[0], int(encode_batch)):
            part = clips[c0:c0 + int(encode_batch)]
            parts.append(self._encode(video=part, video_mask=ones[:part.shape[0]])['visual_output'])
        visual = parts[0] if len(parts) == 1 else torch.cat(parts, 0)
        if visual.dim() != 3 or visual.shape[1] * fd != T:
            raise ValueError("FeatureGallery.add_windows: the encoder gave features %s for clips of %d frames, not %d segments "
                             "of %d frames" % (tuple(visual.shape), T, T // fd, fd))
        return self._add_window_features(visual.reshape(b, F // fd, visual.shape[2]), table, group)

    # ------------------------------------------------------------------ removing rows: the live mask, on the host
    @staticmethod
    def _pack_words(flags):
        """bool [n] -> int32 [ceil(n / 32)], bit b of word w = flag 32 w + b (the ops' mask format)"""
        flags = np.asarray(flags, dtype=bool)
        padded = np.zeros(T.mask_words(flags.shape[0]) * 32, dtype=bool)
        padded[:flags.shape[0]] = flags
        return np.packbits(padded, bitorder="little").view("<i4").astype(np.int32)

    def _forget_removals(self):
        self._live_host, self._live_dev, self._live_count = None, None, 0

    def _upload_live(self, w0, w1):
        """words [w0, w1) of the live mask, computed from the host mirror, to the device buffer (which grows with the rows)"""
        need = T.mask_words(max(self._rows.shape[0], self._n, 1))
        dev = getattr(self, "_live_dev", None)
        if dev is None or dev.shape[0] < need:
            self._live_dev = torch.zeros(need, device=self.device, dtype=torch.int32)
            w0, w1 = 0, T.mask_words(self._n)
        if w1 > w0:
            self._live_dev[w0:w1] = self._host_to_device(self._pack_words(self._live[32 * w0:32 * w1]))

    def _live_words(self):
        """the live mask over the positions in use, int32 [ceil(span / 32)] on the device"""
        return self._live_dev[:T.mask_words(self._n)]

    def _positions(self, positions, what):
        """int / host sequence / CPU LongTensor -> int64 array of distinct positions inside [0, span): checks only"""
        if torch.is_tensor(positions):
            if positions.device.type != "cpu" or positions.dtype != torch.int64:
                raise ValueError("FeatureGallery.%s: positions are an int, a host sequence or a CPU LongTensor, not a %s %s "
                                 "tensor (reading a device tensor would synchronise)" % (what, positions.device, positions.dtype))
            pos = positions.numpy().reshape(-1) if positions.dim() <= 1 else None
        elif isinstance(positions, (int, np.integer)):
            pos = np.array([int(positions)])
        else:
            pos = np.asarray(list(positions))
            pos = pos if pos.ndim == 1 and (pos.size == 0 or pos.dtype.kind in "iu") else None
        if pos is None:
            raise ValueError("FeatureGallery.%s: positions are one int or a flat sequence of ints" % what)
        pos = pos.astype(np.int64)
        if pos.size and (pos.min() < 0 or pos.max() >= self._n):
            raise ValueError("FeatureGallery.%s: position %d is outside [0, %d)"
                             % (what, int(pos[(pos < 0) | (pos >= self._n)][0]), self._n))
        if np.unique(pos).size != pos.size:
            raise ValueError("FeatureGallery.%s: a position is listed twice" % what)
        return pos

    def remove(self, positions):
        """Take rows out: ``search*`` no longer ranks them, ``similarity*`` shows -inf in their columns.  ``positions``: an
        int, a host sequence or a CPU LongTensor (never a device tensor: no synchronisation).  The other rows keep their
        positions and rows added later get new ones behind ``span`` - ``compact()`` closes the holes.  A position outside
        [0, span), already removed or listed twice: ValueError, nothing changed."""
        pos = self._positions(positions, "remove")
        live = self._live
        if live is not None and pos.size and not live[pos].all():
            raise ValueError("FeatureGallery.remove: position %d is already removed" % int(pos[~live[pos]][0]))
        if pos.size == 0:
            return
        if live is None:
            self._live_host, self._live_dev, self._live_count = np.ones(self._n, dtype=bool), None, self._n
        self._live_host[pos] = False
        self._live_count -= int(pos.size)
        if getattr(self, "_live_dev", None) is None:
            self._upload_live(0, T.mask_words(self._n))
        else:                                                    # one upload: the words from the first to the last changed one
            self._upload_live(int(pos.min()) >> 5, (int(pos.max()) >> 5) + 1)
        if self._grouped and self._open is not None and not self._live_host[self._open[1]:].any():
            self._closed.add(self._open[0])                      # the last group is gone: rows added next start a new one,
            self._open = None                                    # and its label stays refused like any other held label

    @staticmethod
    def _label_list(labels, what):
        """an int, a host sequence or a CPU LongTensor of labels -> int64 array (a device tensor would have to be read)"""
        if torch.is_tensor(labels):
            if labels.device.type != "cpu" or labels.dtype != torch.int64:
                raise ValueError("FeatureGallery.%s: labels are an int, a host sequence or a CPU LongTensor, not a %s %s tensor "
                                 "(reading a device tensor would synchronise)" % (what, labels.device, labels.dtype))
            return labels.numpy().reshape(-1).astype(np.int64)
        if isinstance(labels, (int, np.integer)):
            return np.array([int(labels)], dtype=np.int64)
        lab = np.asarray(list(labels))
        if lab.ndim != 1 or (lab.size and lab.dtype.kind not in "iu"):
            raise ValueError("FeatureGallery.%s: labels are one int or a flat sequence of ints" % what)
        return lab.astype(np.int64)

    def remove_groups(self, labels):
        """grouped=True: ``remove`` all rows still held of the groups with these labels (an int, a host sequence or a CPU
        LongTensor - never a device tensor).  A label
        no row held carries: ValueError, nothing changed.  The labels stay refused by ``add`` until ``compact()``."""
        self._need_grouped("remove_groups")
        want = np.unique(self._label_list(labels, "remove_groups"))
        held = self.labels.numpy()
        hit = np.isin(held, want) & (self._live if self._live is not None else True)
        missing = np.setdiff1d(want, held[hit])
        if missing.size:
            raise ValueError("FeatureGallery.remove_groups: no row held has the label %d" % int(missing[0]))
        self.remove(np.flatnonzero(hit))

    def row_mask(self, positions=None, groups=None):
        """A mask for ``allow=``, built on the host: int32 [ceil(span / 32)] on the device with the bits of ``positions`` (as
        ``remove`` takes them) and of the rows of the groups labelled ``groups`` (grouped=True) set; neither: every position.
        Build it once per subset - a tenant, a channel - and pass it to any number of searches; it describes the positions in
        use now (a mask built before rows were added lacks their bits, and after ``compact()`` it is stale)."""
        flags = np.zeros(self._n, dtype=bool)
        if positions is None and groups is None:
            flags[:] = True
        if positions is not None:
            flags[self._positions(positions, "row_mask")] = True
        if groups is not None:
            self._need_grouped("row_mask")
            want = self._label_list(groups, "row_mask")
            held = self.labels.numpy()
            missing = np.setdiff1d(want, held)
            if missing.size:
                raise ValueError("FeatureGallery.row_mask: no row has the label %d" % int(missing[0]))
            flags |= np.isin(held, want)
        words = self._pack_words(flags)
        return self._host_to_device(words) if words.size else torch.zeros(0, device=self.device, dtype=torch.int32)

    def compact(self):
        """Drop the removed rows, keep the order of the others -> CPU LongTensor [old span]: every row's new position, -1 for
        the removed ones.  Afterwards the gallery is, bit for bit, the one to which only the surviving rows were added in
        that order (statistics and labels move with their rows, the groups are rebuilt from the surviving labels, removed
        labels are free again).  One index_select per buffer with an index computed on the host: no new kernel, no
        synchronisation.  Nothing removed: nothing happens."""
        live, old = self._live, self._n
        if live is None:
            return torch.arange(old)
        keep = np.flatnonzero(live)
        cnt = int(keep.size)
        new_pos = np.full(old, -1, dtype=np.int64)
        new_pos[keep] = np.arange(cnt)
        labels = self.labels[torch.from_numpy(keep)] if self._grouped else None
        if self._window_records() is not None:
            self._win_host = self._window_records()[keep]
        if cnt:
            index = self._host_to_device(keep)
            for name in ("_rows",) + (("_m", "_s") if self._dsl else ()):
                buf = getattr(self, name)
                buf[:cnt] = buf.index_select(0, index)           # (index_select copies first: no overlap)
        self._n = cnt
        self._forget_removals()
        if self._grouped:
            self._reset_groups()
            self._take_groups(self._plan_groups(labels, 0, cnt), 0, cnt)
        return torch.from_numpy(new_pos)

    def _allow_words(self, allow, nq):
        """``allow=`` of a search over nq queries -> None, or the mask the ranking sees (``allow & live``): int32 [W] or [nq, W]"""
        words, live = T.mask_words(self._n), None if self._live is None else self._live_words()
        if allow is None:
            return live
        if not torch.is_tensor(allow) or allow.device != self._rows.device:
            raise ValueError("FeatureGallery: allow= is a tensor on the gallery's device (an int32 mask [W] or [Nq, W], a bool "
                             "tensor [span] or [Nq, span], or what row_mask() returns)")
        if allow.dim() not in (1, 2) or (allow.dim() == 2 and allow.shape[0] != nq):
            raise ValueError("FeatureGallery: allow= %s is neither one mask nor one per query (%d)" % (tuple(allow.shape), nq))
        if allow.dtype == torch.bool:
            if allow.shape[-1] != self._n:
                raise ValueError("FeatureGallery: a bool allow= has one flag per position in use (%d), not %d"
                                 % (self._n, allow.shape[-1]))
            if self._n == 0:
                return None                                      # (no position in use: nothing to pack, the search gives the fill)
            packed = torch.ops.centerclip.pack_row_mask(allow)
            allow = packed[0] if allow.dim() == 1 else packed
        elif allow.dtype != torch.int32:
            raise ValueError("FeatureGallery: allow= is int32 mask words or bool flags, not %s" % allow.dtype)
        if allow.shape[-1] < words:
            raise ValueError("FeatureGallery: allow= holds %d words, the %d positions in use need %d"
                             % (allow.shape[-1], self._n, words))
        allow = allow[..., :words]
        return (allow if live is None else allow & live).contiguous()

    # ------------------------------------------------------------------ asking
    def _mult(self):
        return T.logit_multiplier(self.core._logit_scale_value())

    def _query_rows(self, features, mask):
        return self._text_rows(features) if self.side == "video" else self._video_rows(features, mask)

    def _check_list(self, k, after, nq, what):
        """the refusals of a list's length and cursor, which need nothing encoded: 1 <= k <= 4096; ``after`` is None or a pair
        (scores fp32 [nq], positions int32 / int64 [nq]) of tensors on the gallery's device, passed through unread"""
        if not 1 <= int(k) <= T.TOPK_DEEP_MAXK:
            raise ValueError("FeatureGallery.%s: 1 <= k <= %d, not %d" % (what, T.TOPK_DEEP_MAXK, int(k)))
        if after is None:
            return
        if not isinstance(after, (tuple, list)) or len(after) != 2 or not all(torch.is_tensor(a) for a in after):
            raise ValueError("FeatureGallery.%s: after= is a pair (scores, positions) of device tensors, typically the last "
                             "column of an earlier result" % what)
        scores, pos = after
        if (scores.dtype != torch.float32 or pos.dtype not in (torch.int32, torch.int64) or tuple(scores.shape) != (nq,)
                or tuple(pos.shape) != (nq,) or scores.device != self._rows.device or pos.device != self._rows.device):
            raise ValueError("FeatureGallery.%s: after= holds scores %s %s on %s and positions %s %s on %s, not one fp32 score and "
                             "one int32 / int64 position per query (%d) on %s (a host value would have to be uploaded: pass the "
                             "columns of the earlier result)" % (what, tuple(scores.shape), scores.dtype, scores.device,
                                                                 tuple(pos.shape), pos.dtype, pos.device, nq, self._rows.device))

    def _softmax_args(self, q):
        """(m, s, stats_on_gallery, n_total) of every ranking of the queries q: the dual softmax's statistics - side="video":
        the gallery rows' pairs over the bank; side="text": the queries' pairs over the captions held, taken once per call -
        or (None, None, ., 0) for the plain score"""
        on_gallery = int(self.side == "video")
        if not self._dsl:
            return None, None, on_gallery, 0
        if on_gallery:
            return self._m, self._s, 1, self._bank.shape[0]
        return self._query_stats(q) + (0, len(self))

    def _search_rows(self, q, k, groups=False, allow=None, after=None):
        """the k best rows - groups: the best row of each of the k best groups - of every row of q; after ``remove`` or with
        ``allow=``: of the rows both leave selectable; ``after``: of those behind that entry of the ordering"""
        k = int(k)
        if self._dsl:
            self._need_bank()
        mask = self._allow_words(allow, q.shape[0])
        if len(self) == 0:                                  # nothing to rank: the fill of a list longer than the gallery
            return (torch.full((q.shape[0], k), float("-inf"), device=self.device),
                    torch.full((q.shape[0], k), -1, device=self.device, dtype=torch.int64))
        return torch.ops.centerclip.similarity_topk_deep(q, self._rows, self._n, self._mult(), self.products, k, mask,
                                                         *self._softmax_args(q), self._head if groups else None,
                                                         *(after if after is not None else (None, None)))

    def _search_group_rows(self, q, k, allow=None, after=None):
        scores, pos = self._search_rows(q, k, groups=True, allow=allow, after=after)
        return scores, self._label_dev[pos], pos                 # (position -1, the fill: the last entry, -1)

    def search_groups(self, *inputs, k=10, allow=None, after=None):
        """grouped=True: the queries of ``search`` -> (scores [Nq, k] fp32, labels [Nq, k] int64, positions [Nq, k] int64) of
        the k best groups, best first, each by its best row (``positions``); (-inf, -1, -1) beyond the number of groups.
        After ``remove`` / with ``allow=`` (see ``search``): a group is ranked by its best selectable row, one without any
        does not appear.  ``after=(scores[:, -1], positions[:, -1])`` of an earlier result: the k groups behind it (see
        ``search``; the position is the group's best row)."""
        self._need_grouped("search_groups")
        self._check_list(k, after, inputs[0].shape[0], "search_groups")      # (refusals come before anything is encoded)
        return self._search_group_rows(self._encode_text(*inputs) if self.side == "video" else self._encode_video(*inputs), k,
                                       allow, after)

    def search_groups_features(self, features, k=10, mask=None, allow=None, after=None):
        """``search_groups`` for query features computed elsewhere (as ``search_features``)."""
        self._need_grouped("search_groups_features")
        self._check_list(k, after, features.shape[0], "search_groups_features")
        return self._search_group_rows(self._query_rows(features, mask), k, allow, after)

    def search(self, *inputs, k=10, allow=None, after=None):
        """``search(input_ids, k=10)`` (``search(video, video_mask, k=10)`` for side="text") -> (scores [Nq, k] fp32, positions
        [Nq, k] int64), best first, equal scores by smaller position; (-inf, -1) beyond the gallery's size.  Removed rows are
        not ranked.  ``allow=``: rank a subset only - an int32 mask [W] or [Nq, W] on the device (bit b of word w = position
        32 w + b, W >= ceil(span / 32)), a device bool tensor [span] or [Nq, span], or what ``row_mask`` returns; one mask
        for all queries also skips the tiles of 16 rows it leaves empty.  The fill starts behind the selectable rows.
        1 <= k <= 4096: beyond 128 the list is built in pages of at most 128, each one more pass over the gallery.
        ``after=(scores [Nq], positions [Nq])``, device tensors - typically ``(scores[:, -1], positions[:, -1])`` of an earlier
        result: the k entries that FOLLOW that pair in the full ordering (after the fill (-inf, -1): only fill), whatever
        happened to the pair's row since - the cursor of a "next page" that needs no state and stays right when rows are
        removed between two pages (not across ``compact()``, which renumbers).  Nothing here is read on the host."""
        self._check_list(k, after, inputs[0].shape[0], "search")             # (refusals come before anything is encoded)
        return self._search_rows(self._encode_text(*inputs) if self.side == "video" else self._encode_video(*inputs), k,
                                 allow=allow, after=after)

    def search_features(self, features, k=10, mask=None, allow=None, after=None):
        """``search`` for query features computed elsewhere (sequence_output; side="text": visual_output and its mask)."""
        self._check_list(k, after, features.shape[0], "search_features")
        return self._search_rows(self._query_rows(features, mask), k, allow=allow, after=after)

    # ------------------------------------------------------------------ the rank of a known row or group
    def _targets(self, target, nq, what):
        """one position per query -> int tensor [nq] on the device.  A host int sequence / CPU LongTensor is checked against
        [0, span) before anything is launched (the same position may serve several queries); a device integer tensor is
        passed through unread"""
        if torch.is_tensor(target) and target.device.type != "cpu":
            if target.dtype not in (torch.int32, torch.int64) or target.dim() != 1 or target.shape[0] != nq:
                raise ValueError("FeatureGallery.%s: target %s %s is not one int32 / int64 position per query (%d)"
                                 % (what, tuple(target.shape), target.dtype, nq))
            return target
        what = "FeatureGallery." + what
        pos = _exactly(_host_ints(target, what, "targets"), nq, what, "targets", "query")
        if pos.size and (pos.min() < 0 or pos.max() >= self._n):
            raise ValueError("%s: target %d is outside [0, %d)" % (what, int(pos[(pos < 0) | (pos >= self._n)][0]), self._n))
        return self._host_to_device(pos)

    def _group_targets(self, target, nq):
        """one group label per query (host values) -> the positions of the groups' heads, through the host label mirror"""
        want = _exactly(_host_ints(target, "FeatureGallery.rank_groups", "labels"), nq, "FeatureGallery.rank_groups",
                        "target labels", "query")
        heads = self._group_heads(want)
        if (heads < 0).any():
            raise ValueError("FeatureGallery.rank_groups: no row held has the label %d" % int(want[heads < 0][0]))
        return heads

    def _group_heads(self, want):
        """labels int64 [n] -> the positions of their groups' heads, -1 for a label no row carries (it never raises: a shard
        of a ShardedGallery is asked for labels another shard holds)"""
        held = self.labels.numpy()                               # (removed rows keep their label until compact())
        first = np.flatnonzero(np.concatenate(([True], held[1:] != held[:-1]))) if held.size else np.zeros(0, dtype=np.int64)
        head_of = dict(zip(held[first].tolist(), first.tolist()))                      # (a label never returns: one label, one run)
        return np.array([head_of.get(v, -1) for v in want.tolist()], dtype=np.int64)

    def _rank_rows(self, q, target, groups=False, allow=None):
        """(ranks int64 [Nq], scores fp32 [Nq], counts int32 [Nq, 3]) of the targets among the rows (groups) ``_search_rows``
        ranks, with its choices of statistics"""
        if self._dsl:
            self._need_bank()
        mask = self._allow_words(allow, q.shape[0])
        counts, scores = torch.ops.centerclip.similarity_rank(q, self._rows, self._n, self._mult(), self.products, target, mask,
                                                              *self._softmax_args(q), self._head if groups else None)
        return counts[:, 0].to(torch.int64) + counts[:, 2], scores, counts

    def rank(self, *inputs, target, allow=None):
        """Where a known row stands: the queries of ``search`` and one ``target`` position per query -> (ranks int64 [Nq],
        scores fp32 [Nq], counts int32 [Nq, 3]), all on the device.  ``ranks[q]`` is the 0-based place of row ``target[q]`` in
        ``search``'s full ordering for query q (so ``search(k)[1][q, ranks[q]] == target[q]`` whenever ranks[q] < k), for any
        place, not only the first 128; ``scores[q]`` the pair's score, ``search``'s bits; ``counts[q]`` = (rows with a greater
        score, with an equal score - the target included -, with an equal score and a smaller position): what R@k, MdR and
        MnR are made of.  ``target``: a host int sequence or a CPU LongTensor, checked against [0, span) before anything is
        launched (one position may serve several queries), or a device integer tensor, passed through without a look (a
        position outside [0, span) then gives counts (0, 0, 0) and score -inf).  Removed rows and ``allow=`` act as in
        ``search``; a target that is itself removed or not allowed keeps its score and is simply not counted: ranks[q] is then
        the place it would take among the selectable rows."""
        target = self._targets(target, inputs[0].shape[0], "rank")           # (refusals come before anything is encoded)
        return self._rank_rows(self._encode_text(*inputs) if self.side == "video" else self._encode_video(*inputs), target,
                               allow=allow)

    def rank_features(self, features, target, mask=None, allow=None):
        """``rank`` for query features computed elsewhere (as ``search_features``)."""
        target = self._targets(target, features.shape[0], "rank_features")
        return self._rank_rows(self._query_rows(features, mask), target, allow=allow)

    def rank_groups(self, *inputs, target, allow=None):
        """grouped=True: where a known GROUP stands among the groups ``search_groups`` ranks.  ``target``: one group label per
        query (an int, a host sequence or a CPU LongTensor - never a device tensor); a label no held row carries: ValueError.
        -> (ranks, scores, counts) as ``rank``, counted over the groups with a selectable row: scores[q] is the group's best
        selectable row (-inf without one), counts[q] = (groups with a greater score, with an equal score, with an equal score
        lying in front of the target's)."""
        self._need_grouped("rank_groups")
        target = self._host_to_device(self._group_targets(target, inputs[0].shape[0]))
        return self._rank_rows(self._encode_text(*inputs) if self.side == "video" else self._encode_video(*inputs), target,
                               groups=True, allow=allow)

    def rank_groups_features(self, features, target, mask=None, allow=None):
        """``rank_groups`` for query features computed elsewhere."""
        self._need_grouped("rank_groups_features")
        target = self._host_to_device(self._group_targets(target, features.shape[0]))
        return self._rank_rows(self._query_rows(features, mask), target, groups=True, allow=allow)

    def _matrix(self, q):
        n = self._n
        if self.side == "video":
            text, video, n_video = q, self._rows[:n], n
        else:
            text, video, n_video = self._rows[:n], q, q.shape[0]
        padded = torch.zeros((max(n_video, self.backend.video_operand_rows(n_video)), 3 * self.E), device=self.device,
                             dtype=torch.float16)
        padded[:n_video] = video
        sim = self.backend.dot_operands(text, padded, n_video, self._mult())
        if self._dsl:                                            # the checking path: the matrix, then the rewrite in place
            self._need_bank()
            m, s = (self._m[:n], self._s[:n]) if self.side == "video" else self._query_stats(q)
            torch.ops.centerclip.dsl_apply_(sim, m.contiguous(), s.contiguous(),
                                            self._bank.shape[0] if self.side == "video" else len(self))
        sim = sim if self.side == "video" else sim.t().contiguous()
        if self._live is not None:                               # removed rows: -inf in their columns
            sim.masked_fill_(~self._host_to_device(self._live.copy())[None, :], float("-inf"))
        return sim

    def similarity(self, *inputs):
        """The whole [Nq, len(self)] matrix of the queries ``search`` takes, through the matrix op of eval_epoch (on a zero-
        padded copy of the video side, as that op requires): for small galleries and for checking ``search``.  With
        dual_softmax=True: D, by ``dsl_apply_`` on that matrix with the statistics ``search`` uses."""
        return self._matrix(self._encode_text(*inputs) if self.side == "video" else self._encode_video(*inputs))

    def similarity_features(self, features, mask=None):
        return self._matrix(self._query_rows(features, mask))

    # ------------------------------------------------------------------ persistence
    def state_dict(self):
        state = {"rows": self._rows[:self._n].clone(), "count": self._n, "E": self.E, "side": self.side,
                 "products": self.products}
        if self._live is not None:                               # (one key more, only after a remove: positions still held)
            state["live"] = torch.from_numpy(self._live.copy())
        if self._dsl:                                            # (a plain gallery's keys are what they were)
            state.update(dual_softmax=True, bank=None if self._bank is None else self._bank.clone(),
                         m=self._m[:self._n].clone(), s=self._s[:self._n].clone())
        if self._grouped:                                        # (the same: three keys more, only here)
            state.update(grouped=True, group_head=self._head[:self._n].clone(), labels=self.labels.clone())
        if self._window_records() is not None:                   # (one key more, only once a window row exists)
            state["windows"] = torch.from_numpy(self._window_records().copy())
        return state

    def load_state_dict(self, state):
        """Replace the contents with a saved gallery's.  E or side that differ from this gallery's: ValueError, nothing
        written; the same for a plain gallery's state into a dual_softmax=True gallery, or the reverse.  The saved ``products``
        are taken over - with dual_softmax=True the bank and the statistics too - so the loaded gallery answers with the saved
        one's bits.  A grouped=True gallery's state into a plain one, or the reverse: ValueError, nothing written; the groups
        are rebuilt from the saved labels."""
        rows, count = state["rows"], int(state["count"])
        if bool(state.get("grouped", False)) != self._grouped:
            raise ValueError("FeatureGallery.load_state_dict: saved grouped=%s, this gallery grouped=%s"
                             % (bool(state.get("grouped", False)), self._grouped))
        if bool(state.get("dual_softmax", False)) != self._dsl:
            raise ValueError("FeatureGallery.load_state_dict: saved dual_softmax=%s, this gallery dual_softmax=%s"
                             % (bool(state.get("dual_softmax", False)), self._dsl))
        if int(state["E"]) != self.E or state["side"] != self.side:
            raise ValueError("FeatureGallery.load_state_dict: saved (E=%s, side=%r), this gallery (E=%d, side=%r)"
                             % (state["E"], state["side"], self.E, self.side))
        if rows.dim() != 2 or tuple(rows.shape) != (count, 3 * self.E) or rows.dtype != torch.float16:
            raise ValueError("FeatureGallery.load_state_dict: rows %s %s do not match count %d, E %d"
                             % (tuple(rows.shape), rows.dtype, count, self.E))
        live = state.get("live")
        if live is not None and (not torch.is_tensor(live) or live.dtype != torch.bool or tuple(live.shape) != (count,)):
            raise ValueError("FeatureGallery.load_state_dict: live is a bool tensor of %d entries" % count)
        windows = state.get("windows")
        if windows is not None and (not torch.is_tensor(windows) or windows.dtype != torch.int64
                                    or tuple(windows.shape) != (count, 2)):
            raise ValueError("FeatureGallery.load_state_dict: windows is a LongTensor [%d, 2]" % count)
        backend = HipBackend.with_products(int(state["products"]))
        if self._dsl:
            bank, m, s = state["bank"], state["m"], state["s"]
            if bank is not None and (bank.dim() != 2 or bank.shape[1] != 3 * self.E or bank.dtype != torch.float16):
                raise ValueError("FeatureGallery.load_state_dict: bank rows %s %s, E %d" % (tuple(bank.shape), bank.dtype, self.E))
            if tuple(m.shape) != (count,) or tuple(s.shape) != (count,) or m.dtype != torch.float32 or s.dtype != torch.float32:
                raise ValueError("FeatureGallery.load_state_dict: statistics %s, %s do not match count %d"
                                 % (tuple(m.shape), tuple(s.shape), count))
        labels = None
        if self._grouped:
            labels, head = state["labels"], state["group_head"]
            if (not torch.is_tensor(labels) or tuple(labels.shape) != (count,) or labels.dtype != torch.int64
                    or tuple(head.shape) != (count,) or head.dtype != torch.int32):
                raise ValueError("FeatureGallery.load_state_dict: labels / group_head do not match count %d" % count)
            labels = labels.cpu()
            kept = (self._label_chunks, self._closed, self._open, self._groups)
            self._reset_groups()
            try:
                self._plan_groups(labels, 0, count)              # (a label that returns: refused before anything is written)
            except ValueError:
                self._label_chunks, self._closed, self._open, self._groups = kept
                raise
        if self._dsl:
            self._bank = None                                    # (the saved statistics are taken over, not recomputed)
        self._n = 0
        self._forget_removals()
        self._append(rows.to(self.device), labels)
        self._win_host = None if windows is None else windows.cpu().numpy().copy()
        self.products, self.backend = int(state["products"]), backend
        if self._dsl:
            self._bank = None if bank is None else bank.to(self.device).clone()
            self._m[:count], self._s[:count] = m.to(self.device), s.to(self.device)
        if self._grouped:
            self._head[:count] = head.to(self.device)            # (what the labels give; the saved array is taken over)
        if live is not None:
            self.remove(np.flatnonzero(~live.cpu().numpy()))


__all__ = ["FeatureGallery"]
