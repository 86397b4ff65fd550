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
"""
import torch

from . import _lib as L
from . import torch_ops as T
from .eval import HipBackend, _video_operand

SIDES = ("video", "text")


class FeatureGallery:
    """``side``: what the gallery holds - "video" (queries are captions) or "text" (queries are clips).  ``capacity``: rows
    to allocate up front; the buffer grows geometrically and keeps its rows bit for bit.  ``products``: the fp16 products per
    multiply-add of a score (``HipBackend.with_products``); None = ``HipBackend.similarity_products``.  The scores are
    exp(logit_scale) * cosine as in ``eval._similarity_matrix``; a ``camoe_dsl`` model is refused: the dual softmax needs
    column statistics over all queries and is no per-query ranking."""

    def __init__(self, model, side="video", capacity=0, products=None):
        if side not in SIDES:
            raise ValueError("FeatureGallery: side is 'video' or 'text', not %r" % (side,))
        core = model.module if hasattr(model, 'module') else model
        if getattr(core, "camoe_dsl", False):
            raise ValueError("FeatureGallery: camoe_dsl ranks S * softmax(S, dim=0) * Nt, which depends on every query at once")
        products = HipBackend.similarity_products if products is None else int(products)
        self.backend = HipBackend.with_products(products)        # (raises for anything but 1, 2, 3)
        self.device = next(core.parameters()).device
        if self.device.type != "cuda":
            raise L.CenterClipHipError("FeatureGallery runs on MI355X only: the model is on %s (no CPU fallback)" % self.device)
        self.model, self.core, self.side, self.products = model, core, side, products
        self.E = int(core.clip_config['embed_dim'])
        self._rows = torch.zeros((max(int(capacity), 0), 3 * self.E), device=self.device, dtype=torch.float16)
        self._n = 0

    def __len__(self):
        return self._n

    def clear(self):
        self._n = 0

    @property
    def rows(self):
        """The operand rows held, [len(self), 3E] fp16 (a view of the buffer)."""
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
    def _append(self, rows):
        if rows.dim() != 2 or rows.shape[1] != 3 * self.E:
            raise ValueError("FeatureGallery: operand rows of width %d, the model's embed_dim gives %d"
                             % (rows.shape[-1], 3 * self.E))
        start, n = self._n, self._n + rows.shape[0]
        if n > self._rows.shape[0]:
            grown = torch.zeros((max(n, 2 * self._rows.shape[0]), 3 * self.E), device=self.device, dtype=torch.float16)
            grown[:start] = self._rows[:start]
            self._rows = grown
        self._rows[start:n] = rows
        self._n = n
        return torch.arange(start, n)

    def add(self, *inputs):
        """``add(video, video_mask)`` (``add(input_ids)`` for side="text"): encode a batch as eval_epoch does and append
        its rows -> the positions they got (LongTensor)."""
        return self._append(self._encode_video(*inputs) if self.side == "video" else self._encode_text(*inputs))

    def add_features(self, features, mask=None):
        """The same for features cached elsewhere: ``add_features(visual_output, video_mask)`` ([b, T', E] per-segment
        features with the loader's mask, or [b, E] pooled rows) or, side="text", ``add_features(sequence_output)``."""
        return self._append(self._video_rows(features, mask) if self.side == "video" else self._text_rows(features))

    # ------------------------------------------------------------------ asking
    def _mult(self):
        return T.logit_multiplier(self.core._logit_scale_value())

    def _query_rows(self, features, mask):
        return self._text_rows(features) if self.side == "video" else self._video_rows(features, mask)

    def _search_rows(self, q, k):
        k = int(k)
        if self._n == 0:                                     # nothing to rank: the fill of a list longer than the gallery
            if not 1 <= k <= 128:
                raise ValueError("FeatureGallery: 1 <= k <= 128")
            return (torch.full((q.shape[0], k), float("-inf"), device=self.device),
                    torch.full((q.shape[0], k), -1, device=self.device, dtype=torch.int64))
        return torch.ops.centerclip.similarity_topk(q, self._rows, self._n, self._mult(), self.products, k)

    def search(self, *inputs, k=10):
        """``search(input_ids, k=10)`` (``search(video, video_mask, k=10)`` for side="text") -> (scores [Nq, k] fp32, positions
        [Nq, k] int64), best first, equal scores by smaller position; (-inf, -1) beyond the gallery's size."""
        return self._search_rows(self._encode_text(*inputs) if self.side == "video" else self._encode_video(*inputs), k)

    def search_features(self, features, k=10, mask=None):
        """``search`` for query features computed elsewhere (sequence_output; side="text": visual_output and its mask)."""
        return self._search_rows(self._query_rows(features, mask), k)

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
        return sim if self.side == "video" else sim.t().contiguous()

    def similarity(self, *inputs):
        """The whole [Nq, len(self)] matrix of the queries ``search`` takes, through the matrix op of eval_epoch (on a zero-
        padded copy of the video side, as that op requires): for small galleries and for checking ``search``."""
        return self._matrix(self._encode_text(*inputs) if self.side == "video" else self._encode_video(*inputs))

    def similarity_features(self, features, mask=None):
        return self._matrix(self._query_rows(features, mask))

    # ------------------------------------------------------------------ persistence
    def state_dict(self):
        return {"rows": self._rows[:self._n].clone(), "count": self._n, "E": self.E, "side": self.side,
                "products": self.products}

    def load_state_dict(self, state):
        """Replace the contents with a saved gallery's.  E or side that differ from this gallery's: ValueError, nothing
        written.  The saved ``products`` are taken over, so the loaded gallery answers with the saved one's bits."""
        rows, count = state["rows"], int(state["count"])
        if int(state["E"]) != self.E or state["side"] != self.side:
            raise ValueError("FeatureGallery.load_state_dict: saved (E=%s, side=%r), this gallery (E=%d, side=%r)"
                             % (state["E"], state["side"], self.E, self.side))
        if rows.dim() != 2 or tuple(rows.shape) != (count, 3 * self.E) or rows.dtype != torch.float16:
            raise ValueError("FeatureGallery.load_state_dict: rows %s %s do not match count %d, E %d"
                             % (tuple(rows.shape), rows.dtype, count, self.E))
        backend = HipBackend.with_products(int(state["products"]))
        self._n = 0
        self._append(rows.to(self.device))
        self.products, self.backend = int(state["products"]), backend


__all__ = ["FeatureGallery"]
