"""Replicate sharding across GPUs/processes and the single reduction step.

The reference's only parallelism is independent replicates (rayon over replicate ids,
src/main.rs:221-224; cluster array jobs with distinct --seed, src/main.rs:213). Here replicates
are split into contiguous global-id ranges, one per rank; because every replicate's RNG stream
is keyed by its GLOBAL id (include/ecdna_ssa.h), per-replicate results are identical for any
number of ranks, and the pooled histogram of a G-rank run is the sum of the shards' histograms —
one all-reduce (RCCL over xGMI on GPUs, gloo in CPU tests). Nothing else is exchanged.
"""
from __future__ import annotations

from typing import Tuple


def shard_range(rank: int, world: int, total: int) -> Tuple[int, int]:
    """Strong scaling: global ids [first, first + n) of `rank` when `total` replicates are split."""
    if not (0 <= rank < world):
        raise ValueError("rank out of range")
    first = rank * total // world
    last = (rank + 1) * total // world
    return first, last - first


def interleaved_range(rank: int, world: int, total: int) -> Tuple[int, int, int]:
    """Strong scaling, interleaved: `rank` runs global ids rank, rank + world, rank + 2 world, ... < total,
    as (first, n, stride) for RunSpec(first_replicate, n_replicates, replicate_stride). Every rank gets
    the same mix of parameter sets, so an ABC sweep whose sets differ in cost (C4: initial copy numbers
    1 .. 128) is balanced across GPUs; contiguous shards would hand each GPU one cost class."""
    if not (0 <= rank < world):
        raise ValueError("rank out of range")
    n = (total - rank + world - 1) // world if total > rank else 0
    return rank, n, world


def weak_range(rank: int, per_rank: int) -> Tuple[int, int]:
    """Weak scaling: every rank runs `per_rank` replicates; rank g owns [g*per_rank, (g+1)*per_rank)."""
    return rank * per_rank, per_rank


def k0_split(spec, k0_min: int, wide_kmax: int, caps: Tuple[int, int]):
    """A bin-store shard split by initial copy number ("C4 shard split"): the replicates whose
    parameter set starts with a cell of k0 >= k0_min copies run on a second context with K = wide_kmax, whose bins
    keep their cells in LDS (with K = 64 most of them sit in the large-k row in HBM), concurrently with the rest;
    caps = (max_workgroups of the rest, of the heavy part) so that the two persistent grids share the GPU. The
    heavy replicates must be a suffix of the shard's local order (the C4 sweep orders its sets by k0). Each
    replicate's results are those of a run at its part's K (bin_kmax orders the cells, so K is part of the draw
    mapping). Returns [(spec, local offset)] of the non-empty parts."""
    import dataclasses

    import numpy as np

    n, first, stride = spec.n_replicates, spec.first_replicate, spec.stride()
    if n == 0:
        return [(spec, 0)]
    if spec.init_per_set is None:
        k0s = [max(spec.init or {1: 1})] * len(spec.rates)
    else:
        k0s = [max(d) if d else 0 for d in spec.init_per_set]
    sets = (first + np.arange(n, dtype=np.int64) * stride) // int(spec.params().reps_per_set)
    heavy = np.asarray(k0s)[sets] >= k0_min
    i0 = int(np.argmax(heavy)) if heavy.any() else n
    if not np.all(heavy[i0:]):
        raise ValueError("k0_split: the heavy replicates are not a suffix of the shard")
    parts = []
    if i0 > 0:
        parts.append((dataclasses.replace(spec, n_replicates=i0, max_workgroups=caps[0], _keep=[]), 0))
    if i0 < n:
        parts.append((dataclasses.replace(spec, first_replicate=first + i0 * stride, n_replicates=n - i0,
                                          bin_kmax=wide_kmax, max_workgroups=caps[1], _keep=[]), i0))
    return parts


def reduce_outputs(hist, totals, group=None) -> None:
    """Sum the per-rank copy-number histograms and totals in place (int64 tensors: u64 counts stay
    far below 2^63). The histogram bins and totals words are plain integer sums, so the result is
    exact and independent of the reduction order."""
    import torch.distributed as dist

    dist.all_reduce(hist, op=dist.ReduceOp.SUM, group=group)
    dist.all_reduce(totals, op=dist.ReduceOp.SUM, group=group)


def rank_ids(rank: int, world: int, total: int, layout: str):
    """The global replicate ids a rank owns under `layout`, as a slice of range(total): "contiguous"
    (shard_range), "interleaved" (interleaved_range) or "weak" (weak_range with total // world each)."""
    if layout == "contiguous":
        first, n = shard_range(rank, world, total)
        return slice(first, first + n)
    if layout == "interleaved":
        first, n, stride = interleaved_range(rank, world, total)
        return slice(first, first + n * stride, stride)
    if layout == "weak":
        first, n = weak_range(rank, total // world)
        return slice(first, first + n)
    raise ValueError(f"unknown shard layout {layout!r}")


def gather_records(local, total: int, layout: str = "contiguous", group=None):
    """All-gather per-replicate records into global replicate order on every rank.

    `local` is a [n_local, W] tensor of this rank's records in its own order (row i = the i-th id of
    rank_ids), on the process group's device (CUDA for RCCL, CPU for gloo). The ABC sweep's rejection
    step (abc.md:38-55) needs every replicate's statistics in one place; this is the one exchange it
    adds beside the histogram all-reduce (a gather of R/G records per rank). Shards differ
    by at most one record, so each rank pads to the largest and one all_gather moves them."""
    import torch
    import torch.distributed as dist

    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    ids = [range(total)[rank_ids(r, world, total, layout)] for r in range(world)]
    if local.shape[0] != len(ids[rank]):
        raise ValueError(f"rank {rank} holds {local.shape[0]} records, its shard has {len(ids[rank])}")
    width = tuple(local.shape[1:])
    cap = max(len(x) for x in ids)
    padded = torch.zeros((cap,) + width, dtype=local.dtype, device=local.device)
    padded[: local.shape[0]] = local
    parts = [torch.empty_like(padded) for _ in range(world)]
    dist.all_gather(parts, padded, group=group)
    out = torch.empty((sum(len(x) for x in ids),) + width, dtype=local.dtype, device=local.device)
    for r in range(world):
        out[rank_ids(r, world, total, layout)] = parts[r][: len(ids[r])]
    return out


def gather_structured(arr, total: int, layout: str = "contiguous", device=None, group=None):
    """gather_records for a numpy structured array (ecdna_rep_summary_t or ecdna_rep_stats_t records as
    abi.SUMMARY_DTYPE / abi.STATS_DTYPE): the records travel as raw bytes, so every field comes back
    bit for bit. One record per replicate, or a row of them ([n][S]: the per-snapshot statistics), which comes
    back as [total][S]. `device`: where the exchange buffers live ("cuda" under RCCL, None = CPU for gloo)."""
    import numpy as np
    import torch

    per_replicate = int(np.prod(arr.shape[1:], dtype=np.int64))
    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(len(arr), per_replicate * arr.dtype.itemsize)
    t = torch.from_numpy(raw.copy())
    if device is not None:
        t = t.to(device)
    g = gather_records(t, total, layout, group).cpu().numpy()
    return np.ascontiguousarray(g).view(arr.dtype).reshape((-1,) + tuple(arr.shape[1:]))


class SelectWalk:
    """The rank walk of the 8-bit radix select (select mapping v1, include/ecdna_ssa.h) over digit histograms summed
    over the shards: the walk ecdna_ssa_ctx_select makes on one context (csrc/ssa_select.hpp), in Python, so that a
    sharded sweep finds the global order statistics of its distances from eight small sums instead of a gather of every
    record. Per pass: `prefixes` ([4][K] u64 keys) is the input of every shard's Context.select_digits, and feed() takes
    the sum of their [4][K][256] results. Pass 0's row sum is the population M, which turns fractions into ranks. After
    the eighth feed result() returns the engine.SelectResult."""

    PASSES = 8

    def __init__(self, K: int, ranks=None, fractions=None):
        from .engine import select_ranks

        rk, fr = select_ranks(ranks, fractions)
        if K != (len(rk) if rk is not None else len(fr)):
            raise ValueError(f"K = {K}, but {len(rk) if rk is not None else len(fr)} ranks are given")
        self.K = K
        self.pass_ = 0
        self.population = None
        self._fractions = None if fr is None else [float(f) for f in fr]
        self.ranks = None if rk is None else [int(k) for k in rk]
        self._prefix = [[0] * K for _ in range(4)]
        self._remaining = [[0] * K for _ in range(4)]
        self._less = [[0] * K for _ in range(4)]
        self._count = [[0] * K for _ in range(4)]

    @property
    def prefixes(self):
        import numpy as np

        return np.array(self._prefix, dtype=np.uint64)

    def feed(self, hist) -> None:
        import math

        import numpy as np

        if self.pass_ >= self.PASSES:
            raise ValueError("the walk has had its eight passes")
        hist = np.asarray(hist).astype(np.uint64).reshape(4, self.K, 256)
        if self.pass_ == 0:
            M = self.population = int(hist[0, 0].sum(dtype=np.uint64))
            if self._fractions is not None:  # k = max(1, ceil(f * M)) in f64
                self.ranks = [max(1, int(math.ceil(f * float(M)))) for f in self._fractions]
            self._remaining = [list(self.ranks) for _ in range(4)]
        shift = 56 - 8 * self.pass_
        keep = ((1 << 64) - 1) ^ ((1 << (shift + 8)) - 1)  # the bits above this pass's digit
        for x in range(4):
            for j in range(self.K):
                if self.ranks[j] > self.population:
                    continue
                cum = np.cumsum(hist[x, j], dtype=np.uint64)
                # the smallest digit whose cumulative count reaches the remaining rank
                d = min(int(np.searchsorted(cum, np.uint64(self._remaining[x][j]), side="left")), 255)
                below = int(cum[d - 1]) if d else 0
                self._prefix[x][j] = (self._prefix[x][j] & keep) | (d << shift)
                self._remaining[x][j] -= below
                self._less[x][j] += below
                self._count[x][j] = int(hist[x, j, d])
        self.pass_ += 1

    def result(self):
        import numpy as np

        from .engine import SelectResult

        if self.pass_ != self.PASSES:
            raise ValueError(f"the walk has had {self.pass_} of its {self.PASSES} passes")
        M = self.population
        keys = np.array(self._prefix, dtype=np.uint64)
        sign = np.uint64(1 << 63)
        bits = np.where(keys & sign != 0, keys ^ sign, ~keys)  # the key map's inverse
        values = bits.view(np.float64).copy()
        counts_le = np.array(self._less, dtype=np.uint64) + np.array(self._count, dtype=np.uint64)
        over = np.array(self.ranks, dtype=object) > M
        values[:, over] = np.inf
        counts_le[:, over] = M
        return SelectResult(M, np.array(self.ranks, dtype=np.uint64), values, counts_le)


def _sum_over_ranks(arr, group=None, device=None):
    """The sum of a u64 numpy array over the ranks, as u64: one all-reduce of its int64 view (the counts stay far below
    2^63) — integer sums, exact in any order. `device`: where the exchange buffer lives ("cuda" under RCCL, None = CPU
    for gloo)."""
    import numpy as np
    import torch
    import torch.distributed as dist

    t = torch.from_numpy(np.ascontiguousarray(arr).view(np.int64))
    if device is not None:
        t = t.to(device)
    dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    return t.cpu().numpy().view(np.uint64)


def _select_walk(digits, ranks, fractions, group, device):
    """The eight passes of a sharded select: digits(pass_, prefixes) counts this rank's keys, [4][K][256] u64, and one
    all-reduce per pass joins the shards' arrays for the SelectWalk."""
    K = len(ranks) if ranks is not None else len(fractions if fractions is not None else ())
    walk = SelectWalk(K, ranks=ranks, fractions=fractions)
    for p in range(SelectWalk.PASSES):
        walk.feed(_sum_over_ranks(digits(p, walk.prefixes), group, device))
    return walk.result()


def select(ctx, source: int, ranks=None, fractions=None, timepoints=None, group=None, device=None):
    """Context.select over every rank's shard: the exact order statistics of the whole run's distances, the same
    engine.SelectResult on every rank. Per pass each rank counts its own replicates (Context.select_digits) and one
    all-reduce (int64, sum) of the [4][K][256] array joins them: integer sums, exact in any order. Nothing else is
    exchanged. `device`: where the exchange buffer lives ("cuda" under RCCL, None = CPU for gloo)."""
    return _select_walk(lambda p, prefixes: ctx.select_digits(source, p, prefixes, timepoints), ranks, fractions,
                        group, device)


def select_draws(ctx, targets, sample_cells, n_draws: int = 64, first_draw: int = 0, timepoints=None,
                 store: str = "keep", ranks=None, fractions=None, group=None, device=None):
    """Context.select_draws over every rank's shard: the exact order statistics of the distances over the whole run's
    pairs (replicate, thinning draw), the same engine.SelectResult on every rank. It is select() with
    Context.select_draws_digits in the loop: pass 0 makes each shard's keys, and eight all-reduces (int64, sum) of the
    [4][K][256] arrays join the shards. `device` as for select()."""
    return _select_walk(lambda p, prefixes: ctx.select_draws_digits(targets, sample_cells, p, prefixes, n_draws,
                                                                    first_draw, timepoints, store),
                        ranks, fractions, group, device)


def pool_accepted(ctx, threshold: int, group=None, device=None):
    """Context.pool_accepted over every rank's shard: the whole run's posterior predictive histogram
    [n_param_sets][hist_bins] u64, the same on every rank. Each rank pools its own accepted replicates' kept samples
    and one all-reduce (int64, sum) joins the arrays: integer sums, exact in any order. `device` as for select()."""
    return _sum_over_ranks(ctx.pool_accepted(threshold), group, device)


def accept_draws(ctx, targets, sample_cells, thresholds, n_draws: int = 64, first_draw: int = 0, timepoints=None,
                 store: str = "keep", group=None, device=None):
    """Context.accept_draws over every rank's shard: the result's passes are the rank's own replicates', its sums
    [Q][n_param_sets] u64 the whole run's, the same on every rank. One all-reduce (int64, sum) joins the shards' arrays:
    integer sums, exact in any order. `device` as for select()."""
    res = ctx.accept_draws(targets, sample_cells, thresholds, n_draws, first_draw, timepoints, store)
    res.sums = _sum_over_ranks(res.sums, group, device)
    return res


def pool_draws(ctx, targets, sample_cells, thresholds, threshold: int = 0, n_draws: int = 64, first_draw: int = 0,
               timepoints=None, store: str = "keep", group=None, device=None):
    """Context.pool_draws over every rank's shard: the whole run's pooled histograms, thinned
    [n_targets][n_param_sets][hist_bins] and kept [n_slices][n_param_sets][hist_bins] u64, the same on every rank. Each
    rank pools its own replicates and one all-reduce (int64, sum) per array joins them: integer sums, exact in any
    order. `device` as for select()."""
    res = ctx.pool_draws(targets, sample_cells, thresholds, threshold, n_draws, first_draw, timepoints, store)
    res.thinned = _sum_over_ranks(res.thinned, group, device)
    res.kept = _sum_over_ranks(res.kept, group, device)
    return res


def pool_accepted_timepoints(ctx, threshold: int, group=None, device=None):
    """Context.pool_accepted_timepoints over every rank's shard: the whole run's posterior predictive histogram per
    timepoint, [T][n_param_sets][hist_bins] u64, the same on every rank. Each rank pools its own accepted replicates'
    kept timepoint samples and one all-reduce (int64, sum) joins the arrays: integer sums, exact in any order. `device`
    as for select()."""
    return _sum_over_ranks(ctx.pool_accepted_timepoints(threshold), group, device)
