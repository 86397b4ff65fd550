"""A gallery split in shards (not in the reference): ``ShardedGallery`` answers ``search*`` and ``rank*`` over several
``FeatureGallery`` objects - the shards of one process, or one shard per rank of a process group - with the results of the
CONCATENATED gallery: one ``FeatureGallery`` holding shard 0's positions, then shard 1's, and so on, removed positions
included.  Scores bit for bit, counts integer for integer, the same order - equal scores by smaller shard, then smaller local
position - because a pair's score is one fp32 accumulator per (query, row) and does not depend on the buffer the row sits in.
After a sharded encode (``eval_epoch(shard=True)``, ``dist.PackedFeatures``) every rank searches the rows of its own clips:
nothing is gathered onto one device but k entries per query and shard, and the gallery is not bounded by one card's memory.

    sharded = ShardedGallery(shards=[g0, g1, g2])            # in-process: FeatureGallery objects of this process
    sharded = ShardedGallery(local=gallery, distributed=True)  # one shard per rank; every method below is a collective
    ids = sharded.add(video, video_mask)                     # global ids: (shard << 32) | local position
    scores, ids = sharded.search(input_ids, k=10)            # ids int64 global, -1 for the fill
    more = sharded.search(input_ids, k=10, after=(scores[:, -1], ids[:, -1]))
    ranks, scores, counts = sharded.rank(input_ids, target=truth_ids)
    shard, local = ShardedGallery.split(ids)

Global ids do not move when another shard grows.  How the pieces fit ("Sharded gallery"):
  * ``search*``: every shard runs its own ``search*`` with the same k; (scores, positions[, labels]) travel in ONE
    ``dist.all_gather`` (in-process: a stack); ``similarity_topk_merge`` merges the S lists; labels follow through ``src``.
  * cursors: a bound is only a key.  For shard r and a cursor (s, r_t, p_t) the shard gets (s, p_t) if r == r_t; (s, 2^31 - 1) if
    r < r_t - all of its entries with that score were handed out before; (nextafter(s + 0.0, +inf), 2^31 - 1) if r > r_t - all of
    them are still behind (s = +inf there: a NaN score, whose key lies above every score's, so nothing is held back).  Computed on
    the device; a fill cursor (id -1) gives the fill.
  * ``rank*``: ``similarity_target_score`` with the local targets (-1 where this shard is not the owner), all-reduce MAX of the
    scores (with the owner's index in the same tensor), ``similarity_count`` against that score with ``bound_front`` = the
    target's row (its group's head) on the owner, 0 on the shards behind it, 2^31 - 1 on those in front, -1 where nobody owns
    the target; all-reduce SUM of the counts.

Refused with ValueError, out of scope: ``dual_softmax=True`` with ``side="text"`` (its statistics run over the captions of every
shard), and a group whose rows lie on two shards - that one is documented, not checked on each call: ``validate()`` is the
collective that checks it.  The process-group path runs at world size 2 on one GPU over gloo in the tests; it was never run on
multi-GPU hardware."""
import numpy as np
import torch
import torch.distributed as tdist

from . import dist as ccdist
from . import torch_ops as T
from .search import FeatureGallery, _exactly, _host_ints

FRONT_ALL = 2 ** 31 - 1                                          # a position no shard holds: every equal entry lies in front of it


class ShardedGallery:
    """``shards=[g0, g1, ...]``: in-process mode - ``FeatureGallery`` objects of this process (at most 64), which must agree in
    ``side``, ``E``, ``products``, ``dual_softmax`` and ``grouped`` (ValueError otherwise).  Results land on shard 0's device; a
    call does not synchronise with the host.

    ``local=g, distributed=True``: process-group mode - this rank's shard is ``g``, S = ``dist.world_size()``, shard index =
    rank; without a process group it is one shard.  ``search*``, ``rank*``, ``global_len`` and ``validate`` are collectives:
    all ranks call them with the same queries, the same ``k``, the same cursor and the same targets.  The checks of those
    arguments run before the first collective and depend on nothing a rank holds alone, so they fail on all ranks alike;
    ``allow=`` is the local shard's own mask and is checked against the local span (also before the first collective).
    ``set_query_bank*`` must be given the same bank on every rank: a clip's statistics depend on the bank only.

    The methods mirror ``FeatureGallery`` (each with its ``*_features`` twin), with global ids int64 ``(shard << 32) | local
    position`` wherever it has positions (-1: the fill; ``split`` converts back) and:
      * ``add(..., group=, shard=i)``: to shard i (in-process; default 0), to the local shard in process-group mode.
      * ``search* (allow=)``: the local shard's mask, or in-process a list with one mask or None per shard.
      * ``rank(target=)``: global ids - a device int64 tensor or host ints; an id outside every shard gives (0, 0, 0), -inf.
        ``rank_groups(target=)``: labels (host ints); a label nobody holds ranks like a target outside.
      * ``remove(ids)`` / ``remove_groups(labels)`` / ``row_mask`` route to the shards by id (by who holds the label); in
        process-group mode a rank applies what concerns its shard and skips the rest, so all ranks may pass the same list.
      * ``compact()`` renumbers local positions: global ids and cursors do not survive it.
      * ``len()`` / ``span``: sums over the shards of this process; ``global_len()`` the collective form.
      * ``state_dict()``: the shards' own states, per shard.

    Out of scope, refused: ``dual_softmax=True`` with ``side="text"``; a group (a label, removed rows included until
    ``compact()``) whose rows lie on two shards - ``validate()`` checks it, and that the ranks agree in the five settings
    above, and raises on every rank alike."""

    def __init__(self, shards=None, local=None, distributed=False):
        if (shards is None) == (local is None):
            raise ValueError("ShardedGallery: either shards=[FeatureGallery, ...] (in-process) or local=gallery, distributed=True")
        if shards is not None:
            if distributed:
                raise ValueError("ShardedGallery: shards= is the in-process mode; distributed=True takes local=")
            shards = list(shards)
            self.S, self.first = len(shards), 0
        else:
            if not distributed:
                raise ValueError("ShardedGallery: local= is this rank's shard of a process group: pass distributed=True")
            shards = [local]
            self.S, self.first = ccdist.world_size(), ccdist.rank()
        if not shards or not all(isinstance(g, FeatureGallery) for g in shards):
            raise ValueError("ShardedGallery: the shards are FeatureGallery objects, at least one")
        if self.S > T.TOPK_MERGE_MAX_LISTS:
            raise ValueError("ShardedGallery: %d shards, at most %d" % (self.S, T.TOPK_MERGE_MAX_LISTS))
        self.distributed, self.shards = bool(distributed), shards
        settings = [self._settings(g) for g in shards]
        if any(s != settings[0] for s in settings):
            raise ValueError("ShardedGallery: the shards disagree in (side, E, products, dual_softmax, grouped): %s"
                             % sorted(set(settings)))
        self.side, self.E, self.products, self.dual_softmax, self.grouped = settings[0]
        if self.dual_softmax and self.side == "text":
            raise ValueError("ShardedGallery: dual_softmax=True with side='text' is out of scope: the statistics of a query clip "
                             "run over the captions of every shard")
        self.device = shards[0].device

    @staticmethod
    def _settings(g):
        return (g.side, int(g.E), int(g.products), bool(g._dsl), bool(g._grouped))

    # ------------------------------------------------------------------ ids
    @staticmethod
    def split(ids):
        """global ids -> (shard, local position), elementwise, the fill -1 -> (-1, -1); a tensor, an array or an int"""
        if torch.is_tensor(ids):
            return (ids >> 32), torch.where(ids < 0, torch.full_like(ids, -1), ids & 0xFFFFFFFF)
        ids = np.asarray(ids, dtype=np.int64)
        return ids >> 32, np.where(ids < 0, -1, ids & 0xFFFFFFFF)

    def _mine(self):
        """(shard index, gallery) of the shards this process holds"""
        return [(self.first + i, g) for i, g in enumerate(self.shards)]

    def _route(self, ids, what):
        """host global ids -> {shard index: int64 local positions} for the shards of this process; a shard index outside
        [0, S): ValueError (on every rank alike)"""
        ids = _host_ints(ids, "ShardedGallery." + what, "ids")
        shard, local = self.split(ids)
        if ids.size and ((ids < 0).any() or (shard >= self.S).any()):
            raise ValueError("ShardedGallery.%s: id %d names no shard of %d" % (what, int(ids[(ids < 0) | (shard >= self.S)][0]), self.S))
        return {r: local[shard == r] for r, _ in self._mine()}

    # ------------------------------------------------------------------ sizes
    def __len__(self):
        """Rows held by the shards of this process (process-group mode: by this rank); ``global_len()`` sums over the ranks."""
        return sum(len(g) for g in self.shards)

    @property
    def span(self):
        """Positions in use over the shards of this process, removed ones included."""
        return sum(g.span for g in self.shards)

    def global_len(self):
        """Rows held by all shards (a collective in process-group mode)."""
        if not self.distributed:
            return len(self)
        return sum(v[0] for v in ccdist.all_gather_ints([len(self)], self.device))

    # ------------------------------------------------------------------ filling and removing
    def _shard_arg(self, shard, what):
        if self.distributed:
            if shard is not None and int(shard) != self.first:
                raise ValueError("ShardedGallery.%s: in process-group mode a rank adds to its own shard (%d), not %r"
                                 % (what, self.first, shard))
            return self.first, self.shards[0]
        shard = 0 if shard is None else int(shard)
        if not 0 <= shard < self.S:
            raise ValueError("ShardedGallery.%s: shard %d of %d" % (what, shard, self.S))
        return shard, self.shards[shard]

    def add(self, *inputs, group=None, shard=None):
        """``FeatureGallery.add`` on shard ``shard`` (in-process; default 0) or on the local shard -> global ids (LongTensor)."""
        r, g = self._shard_arg(shard, "add")
        return g.add(*inputs, group=group) + (r << 32)

    def add_features(self, features, mask=None, group=None, shard=None):
        r, g = self._shard_arg(shard, "add_features")
        return g.add_features(features, mask, group=group) + (r << 32)

    def remove(self, ids):
        """Take rows out by global id (host ints).  Everything is checked before any shard changes; ids of shards another rank
        holds are skipped."""
        routed = self._route(ids, "remove")
        for r, g in self._mine():
            pos = g._positions(routed[r], "remove")
            if g._live is not None and pos.size and not g._live[pos].all():
                raise ValueError("ShardedGallery.remove: position %d of shard %d is already removed" % (int(pos[~g._live[pos]][0]), r))
        for r, g in self._mine():
            g.remove(routed[r])

    def _held(self, g, live_only):
        held = g.labels.numpy()
        return np.unique(held[g._live] if live_only and g._live is not None else held)

    def _route_labels(self, labels, what, live_only):
        """labels -> {shard index: the ones that shard holds}; in-process a label nobody holds: ValueError"""
        self._need_grouped(what)
        want = np.unique(_host_ints(labels, "ShardedGallery." + what, "labels"))
        routed = {r: np.intersect1d(want, self._held(g, live_only)) for r, g in self._mine()}
        if not self.distributed:
            missing = np.setdiff1d(want, np.concatenate(list(routed.values())) if routed else want)
            if missing.size:
                raise ValueError("ShardedGallery.%s: no row held has the label %d" % (what, int(missing[0])))
        return routed

    def remove_groups(self, labels):
        """grouped=True: remove the rows still held of the groups with these labels, on whichever shard holds them."""
        routed = self._route_labels(labels, "remove_groups", True)
        for r, g in self._mine():
            if routed[r].size:
                g.remove_groups(routed[r])

    def row_mask(self, positions=None, groups=None):
        """Masks for ``allow=``: ``positions`` are global ids, ``groups`` labels; neither: every position.  In-process a list
        with one mask per shard, in process-group mode the local shard's mask."""
        pos = None if positions is None else self._route(positions, "row_mask")
        lab = None if groups is None else self._route_labels(groups, "row_mask", False)
        masks = [g.row_mask(None if pos is None else pos[r], None if lab is None else lab[r]) for r, g in self._mine()]
        return masks[0] if self.distributed else masks

    def compact(self):
        """``FeatureGallery.compact`` on every shard -> the maps old -> new local position (a list in-process, the local map
        in process-group mode).  Global ids and cursors taken before do not survive it."""
        maps = [g.compact() for g in self.shards]
        return maps[0] if self.distributed else maps

    def clear(self):
        for g in self.shards:
            g.clear()

    def set_query_bank(self, input_ids):
        """``FeatureGallery.set_query_bank`` on every shard (process-group mode: every rank passes the same captions)."""
        for g in self.shards:
            g.set_query_bank(input_ids)

    def set_query_bank_features(self, sequence_output):
        for g in self.shards:
            g.set_query_bank_features(sequence_output)

    def state_dict(self):
        """Per shard: {"shards": S, "first": index of the first shard here, "states": the shards' own state_dicts}."""
        return {"shards": self.S, "first": self.first, "states": [g.state_dict() for g in self.shards]}

    def load_state_dict(self, state):
        if int(state["shards"]) != self.S or int(state["first"]) != self.first or len(state["states"]) != len(self.shards):
            raise ValueError("ShardedGallery.load_state_dict: saved %d shards from %d on (%d here), this one %d from %d on (%d)"
                             % (state["shards"], state["first"], len(state["states"]), self.S, self.first, len(self.shards)))
        for g, s in zip(self.shards, state["states"]):
            g.load_state_dict(s)

    def validate(self):
        """The collective check of what is documented rather than checked per call: the shards of all ranks agree in (side, E,
        products, dual_softmax, grouped), and no label (removed rows included until ``compact()``) lies on two shards.
        ValueError on every rank alike."""
        mine = [(r, self._settings(g), self._held(g, False).tolist() if self.grouped else []) for r, g in self._mine()]
        everyone = [mine]
        if self.distributed and ccdist.is_dist() and ccdist.world_size() > 1:
            everyone = [None] * ccdist.world_size()
            tdist.all_gather_object(everyone, mine)
        entries = sorted(e for part in everyone for e in part)
        if any(e[1] != entries[0][1] for e in entries):
            raise ValueError("ShardedGallery.validate: the shards disagree in (side, E, products, dual_softmax, grouped): %s"
                             % sorted({e[1] for e in entries}))
        owner = {}
        for r, _, labels in entries:
            for v in labels:
                if owner.setdefault(v, r) != r:
                    raise ValueError("ShardedGallery.validate: the group labelled %d has rows on shards %d and %d (out of scope: "
                                     "a group lives on one shard)" % (v, owner[v], r))

    # ------------------------------------------------------------------ the two exchanges
    def _gather(self, per_shard):
        """per_shard: for every shard of this process a tuple of tensors [Bq, ...] -> the tuple of [S, Bq, ...] tensors on
        shard 0's device: a stack in-process, ONE packed all_gather in process-group mode"""
        if not self.distributed:
            return tuple(torch.stack([t.to(self.device) for t in ts]) for ts in zip(*per_shard))
        local = per_shard[0]
        got = ccdist.all_gather(*local)
        got = got if isinstance(got, tuple) else (got,)
        return tuple(t.reshape((self.S,) + tuple(l.shape)) for t, l in zip(got, local))

    def _reduce(self, per_shard, op):
        """per_shard: one tensor per shard of this process -> their elementwise "max" / "sum" over all shards"""
        if not self.distributed:
            stacked = torch.stack([t.to(self.device) for t in per_shard])
            return stacked.amax(0) if op == "max" else stacked.sum(0, dtype=stacked.dtype)
        return ccdist.all_reduce_(per_shard[0].contiguous(), op)

    # ------------------------------------------------------------------ checks that need nothing encoded
    def _need_grouped(self, what):
        if not self.grouped:
            raise ValueError("ShardedGallery.%s: only grouped=True shards have groups" % what)

    def _allow_list(self, allow, what):
        """``allow=`` -> one entry (mask or None) per shard of this process"""
        if self.distributed:
            if isinstance(allow, (list, tuple)):
                raise ValueError("ShardedGallery.%s: in process-group mode allow= is the local shard's mask, not a list" % what)
            return [allow]
        if allow is None:
            return [None] * self.S
        if not isinstance(allow, (list, tuple)) or len(allow) != self.S:
            raise ValueError("ShardedGallery.%s: allow= is a list with one mask or None per shard (%d), not %s"
                             % (what, self.S, "%d entries" % len(allow) if isinstance(allow, (list, tuple)) else type(allow).__name__))
        return list(allow)

    def _check_list(self, k, after, nq, what):
        if not 1 <= int(k) <= T.TOPK_DEEP_MAXK:
            raise ValueError("ShardedGallery.%s: 1 <= k <= %d, not %d" % (what, T.TOPK_DEEP_MAXK, int(k)))
        if after is None:
            return
        if not isinstance(after, (tuple, list)) or len(after) != 2 or not all(torch.is_tensor(a) for a in after):
            raise ValueError("ShardedGallery.%s: after= is a pair (scores, global ids) of device tensors, typically the last "
                             "column of an earlier result" % what)
        scores, ids = after
        if (scores.dtype != torch.float32 or ids.dtype != torch.int64 or tuple(scores.shape) != (nq,) or tuple(ids.shape) != (nq,)
                or scores.device != self.device or ids.device != self.device):
            raise ValueError("ShardedGallery.%s: after= holds scores %s %s on %s and ids %s %s on %s, not one fp32 score and one "
                             "int64 global id per query (%d) on %s" % (what, tuple(scores.shape), scores.dtype, scores.device,
                                                                       tuple(ids.shape), ids.dtype, ids.device, nq, self.device))

    def _row_targets(self, target, nq, what):
        """one global id per query -> int64 tensor [nq] on shard 0's device (a device tensor: passed through unread)"""
        if torch.is_tensor(target) and target.device.type != "cpu":
            if target.dtype != torch.int64 or target.dim() != 1 or target.shape[0] != nq:
                raise ValueError("ShardedGallery.%s: target %s %s is not one int64 global id per query (%d)"
                                 % (what, tuple(target.shape), target.dtype, nq))
            return target.to(self.device)
        what = "ShardedGallery." + what
        ids = _exactly(_host_ints(target, what, "targets"), nq, what, "target global ids", "query")
        return self.shards[0]._host_to_device(ids)

    def _label_targets(self, target, nq, what):
        """one label per query (host ints) -> per shard of this process the local heads, int32 on the shard's device, -1 where
        the shard does not hold the label"""
        self._need_grouped(what)
        want = _exactly(_host_ints(target, "ShardedGallery." + what, "labels"), nq, "ShardedGallery." + what, "target labels",
                        "query")
        return [g._host_to_device(g._group_heads(want).astype(np.int32)) for g in self.shards]

    # ------------------------------------------------------------------ asking
    def _encode_queries(self, inputs):
        g = self.shards[0]
        return g._encode_text(*inputs) if self.side == "video" else g._encode_video(*inputs)

    def _shard_cursor(self, after, r, device):
        """the cursor (scores, global ids) as shard r sees it: (scores fp32 [nq], positions int32 [nq]) on its device"""
        s, ids = after[0].to(device), after[1].to(device)
        owner, pos = ids >> 32, ids & 0xFFFFFFFF
        s0 = s + 0.0
        above = torch.where(torch.isposinf(s0), torch.full_like(s0, float("nan")),
                            torch.nextafter(s0, torch.full_like(s0, float("inf"))))
        pos = torch.where(owner == r, pos, torch.full_like(pos, FRONT_ALL))
        pos = torch.where(ids < 0, torch.full_like(pos, -1), pos)                     # the fill: nothing lies behind it
        return torch.where(owner < r, above, s), pos.to(torch.int32)

    def _search_rows(self, q, k, groups, allow, after):
        k, per_shard = int(k), []
        for (r, g), mask in zip(self._mine(), allow):
            qr = q.to(g.device)
            cursor = None if after is None else self._shard_cursor(after, r, g.device)
            scores, pos = g._search_rows(qr, k, groups=groups, allow=mask, after=cursor)
            per_shard.append((scores, pos.to(torch.int32)) + ((g._label_dev[pos],) if groups else ()))
        lists = self._gather(per_shard)
        scores, ids, src = torch.ops.centerclip.similarity_topk_merge(lists[0], lists[1])
        if not groups:
            return scores, ids
        labels = lists[2].permute(1, 0, 2).reshape(q.shape[0], self.S * k)
        labels = labels.gather(1, src.clamp(min=0).to(torch.int64))
        return scores, torch.where(src < 0, torch.full_like(labels, -1), labels), ids

    def search(self, *inputs, k=10, allow=None, after=None):
        """``FeatureGallery.search`` over all shards -> (scores [Nq, k] fp32, global ids [Nq, k] int64), the concatenated
        gallery's list.  ``after=(scores [Nq], global ids [Nq])``: the k entries behind that pair."""
        self._check_list(k, after, inputs[0].shape[0], "search")
        allow = self._allow_list(allow, "search")
        return self._search_rows(self._encode_queries(inputs), k, False, allow, after)

    def search_features(self, features, k=10, mask=None, allow=None, after=None):
        self._check_list(k, after, features.shape[0], "search_features")
        allow = self._allow_list(allow, "search_features")
        return self._search_rows(self.shards[0]._query_rows(features, mask), k, False, allow, after)

    def search_groups(self, *inputs, k=10, allow=None, after=None):
        """``FeatureGallery.search_groups`` over all shards -> (scores, labels, global ids of the groups' best rows)."""
        self._need_grouped("search_groups")
        self._check_list(k, after, inputs[0].shape[0], "search_groups")
        allow = self._allow_list(allow, "search_groups")
        return self._search_rows(self._encode_queries(inputs), k, True, allow, after)

    def search_groups_features(self, features, k=10, mask=None, allow=None, after=None):
        self._need_grouped("search_groups_features")
        self._check_list(k, after, features.shape[0], "search_groups_features")
        allow = self._allow_list(allow, "search_groups_features")
        return self._search_rows(self.shards[0]._query_rows(features, mask), k, True, allow, after)

    # ------------------------------------------------------------------ the rank of a known row or group
    def _rank_rows(self, q, targets, groups, allow):
        """targets: per shard of this process the local target of every query, int32 [nq] on the shard's device, -1 where the
        shard is not the owner -> (ranks int64 [nq], scores fp32 [nq], counts int32 [nq, 3]) on shard 0's device"""
        op, calls, first = torch.ops.centerclip, [], []
        for (r, g), mask, tg in zip(self._mine(), allow, targets):
            if g._dsl:
                g._need_bank()
            qr = q.to(g.device)
            args = (qr, g._rows, g._n, g._mult(), g.products)
            tail = (g._allow_words(mask, qr.shape[0]), *g._softmax_args(qr), g._head if groups else None)
            calls.append((r, args, tail, tg))
            score = op.similarity_target_score(*args, tg, *tail)
            owns = (tg >= 0) & (tg < g._n)
            first.append(torch.stack([score, torch.where(owns, float(r), -1.0).to(torch.float32)]))
        first = self._reduce(first, "max")                                            # the owner's bits, and who it is
        bound, owner = first[0].contiguous(), first[1].to(torch.int32)
        counts = []
        for r, args, tail, tg in calls:
            o = owner.to(tg.device)
            front = torch.where(o == r, tg, torch.where(o < r, torch.zeros_like(tg), torch.full_like(tg, FRONT_ALL)))
            front = torch.where(o < 0, torch.full_like(tg, -1), front)
            counts.append(op.similarity_count(*args, bound.to(tg.device), front, *tail))
        counts = self._reduce(counts, "sum")
        return counts[:, 0].to(torch.int64) + counts[:, 2], bound, counts

    def _local_targets(self, ids):
        out = []
        for r, g in self._mine():
            t = ids.to(g.device)
            pos = t & 0xFFFFFFFF
            out.append(torch.where(((t >> 32) == r) & (pos <= FRONT_ALL), pos, torch.full_like(pos, -1)).to(torch.int32))
        return out

    def rank(self, *inputs, target, allow=None):
        """``FeatureGallery.rank`` over all shards: one global id per query -> (ranks, scores, counts) of the concatenated
        gallery.  An id outside every shard: (0, 0, 0) and -inf."""
        ids = self._row_targets(target, inputs[0].shape[0], "rank")
        allow = self._allow_list(allow, "rank")
        return self._rank_rows(self._encode_queries(inputs), self._local_targets(ids), False, allow)

    def rank_features(self, features, target, mask=None, allow=None):
        ids = self._row_targets(target, features.shape[0], "rank_features")
        allow = self._allow_list(allow, "rank_features")
        return self._rank_rows(self.shards[0]._query_rows(features, mask), self._local_targets(ids), False, allow)

    def rank_groups(self, *inputs, target, allow=None):
        """``FeatureGallery.rank_groups`` over all shards: one label per query (host ints); a label nobody holds ranks like a
        target outside."""
        heads = self._label_targets(target, inputs[0].shape[0], "rank_groups")
        allow = self._allow_list(allow, "rank_groups")
        return self._rank_rows(self._encode_queries(inputs), heads, True, allow)

    def rank_groups_features(self, features, target, mask=None, allow=None):
        heads = self._label_targets(target, features.shape[0], "rank_groups_features")
        allow = self._allow_list(allow, "rank_groups_features")
        return self._rank_rows(self.shards[0]._query_rows(features, mask), heads, True, allow)


__all__ = ["ShardedGallery"]
