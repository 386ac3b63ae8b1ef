"""Cases, float64 reference and census of the hash-grid gradient scatter tests (tests/test_scatter_cases_cpu.py, test_scatter_edges_gpu.py).
Not a test module.

Point placement.  A point case is a ray batch with S = 1 and directions = 0: tn_contract then gives world = origin exactly (o + (0 * se) / 2),
tn_patch_order maps work item i to ray i, so the origin array IS the lane-ordered list of positions and e_bins is arbitrary.  Inside the unit
box p = (o + 2) / 4; with o a multiple of 1/4, p * 16 is an integer: a lattice plane of level 0 (and, on power-of-two grids, of every level).

Reference (`reference_scatter`).  scaled = p32 * res32 in float32 -- the kernel's `px * res` is one IEEE multiply (the library is built with
-ffp-contract=off), and scaled - floor(scaled) is exact in float32 -- then floor and ceil, the hash with the oracle's primes, the eight weights
and the sums in float64 (index_add_).  A is the same scatter of w * |g| (what the error bound is relative to), count the number of
contributions per slot.  Unlike autograd of orc.hash_encode in float64 it does not form p * res in its own precision, so it is the exact sum of
the kernel's own records on grids whose resolutions are no powers of two as well.

Census (`census`).  A restatement of the PLAN only -- seg_plan, bin_plan, plan_replicas, the run-head rule of bin_level, tn_patch_order
(csrc/tn_scatter.hip, tn_common.h) -- that says which edges a case reaches: run lengths per wave, records per (level, bin block, bucket), the
lane-group class of every fold block, chunks, level groups, the binned path's capacity and overflowing buckets, the replicated levels of the
atomic path.  It is used to assert that a case reaches the edge it is named for, never to produce expected values.

Bound (`addends`).  Per slot, with u = 2^-24:  |got - (prefill + ref)| <= (8 + R + F) u A + u |prefill + ref|.
  8  the three `1 - o` roundings, two weight multiplies, the multiply by g and the final double-to-float rounding (one spare);
  R  the longest same-cell run of the case: the run sums are fp32 (0 on the atomic path, whose additions are all counted in F);
  F  the fp32 addends the slot receives through float atomics: 1 where one fold block stores; the fold blocks per bucket where the fold is
     split (segmented: chunks; binned: ceil(records / chunk[level])); count[slot] on the atomic path, without workspace, and (plus the fold
     blocks) for buckets of the binned path that overflow into global atomics.
Prefill.  A float atomic rounds against the slot's running value, prefill included: F addends cost up to F u (|prefill| + A).  The prefill of a
slot the scatter touches is therefore drawn as +-[1, 2) A / count: F |prefill| <= 2 A stays inside the three spare roundings of the bound on
every path, and a slot with one contribution is prefilled at its own magnitude.  Slots the scatter does not touch get U(-1, 1) values that must
come back bit for bit.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch
from torch import Tensor

import thermal_nerfacto_oracle as orc
from nerfstudio_thermal_amd import synth

U = 2.0 ** -24
# constants of the plan (csrc/tn_common.h, csrc/tn_scatter.hip)
BIN_THREADS, FOLD_THREADS = 512, 1024
SLICE_LOG2, MAX_SLICES = 12, 256
SCRATCH_BYTES, REPLICAS = 64 << 20, 16
SPARSE_CHUNK, DENSE_CHUNK, BIN_MAX_COUNTERS = 16384, 32768, 1024
PRIME_Y, PRIME_Z = 2654435761, 805459861

# name -> (levels, log2 of the table size, max_res); base resolution 16
# G8k is there for ONE edge: the floor and the ceil corner of a sample differ by 1 in x, x sits in the low bits of the hash, so the two records
# fall into the same bucket of 4096 slots unless x steps from 4095 to 4096 -- below resolution 4096 every record count per (level, bin block,
# bucket) is even, and the fold's handling of an odd run's half-empty last pair is reached only on a finer grid.  (And with 8 buckets or more:
# the bucket of a corner is the XOR of three bit patterns, and with two bucket bits the 2 x 2 x 2 corners still pair up.)
GRIDS = {"G5": (5, 12, 256), "G16": (16, 14, 2048), "G20": (2, 20, 32), "G8k": (2, 15, 8192)}
RUN_LENGTHS = (1, 2, 3, 4, 5, 8, 9, 15, 16, 17, 31, 32, 33, 48, 63, 64)
RUN_STARTS = (15, 16, 31, 32, 47, 48)
RUNS_P = 2 * 512 + 37


def grid_res(gname: str) -> Tensor:
    L, _, maxr = GRIDS[gname]
    return orc.level_resolutions(L, 16, maxr)


@dataclass
class Case:
    name: str
    grid: str
    N: int
    S: int
    origins: Tensor     # [N, 3] float32
    directions: Tensor  # [N, 3]
    e_bins: Tensor      # [N, S + 1]
    ld: int             # row stride of g_enc, or -1: level-major [L, P, 2]
    want_dpos: bool = False
    marks: Optional[dict] = None  # lanes a case promises something about (lattice)

    @property
    def L(self):
        return GRIDS[self.grid][0]

    @property
    def log2T(self):
        return GRIDS[self.grid][1]

    @property
    def P(self):
        return self.N * self.S

    @functools.cached_property
    def res(self) -> Tensor:
        return grid_res(self.grid)

    @functools.cached_property
    def p32(self) -> Tensor:
        """[P, 3] float32 unit-cube positions in sample order (ray-major), formed operation by operation as tn_contract forms them"""
        smp = orc.Samples(s_bins=self.e_bins, e_bins=self.e_bins)
        p, _ = orc.unit_cube_positions(smp.positions(self.origins, self.directions))
        return p.reshape(-1, 3).contiguous()

    @functools.cached_property
    def g(self) -> Tensor:
        """[P, L, 2] float32 gradient of the encoding"""
        return torch.from_numpy(synth.uniform("sc_g_" + self.name, (self.P, self.L, 2), seed=3))

    def g_enc(self) -> Tensor:
        if self.ld < 0:
            return self.g.permute(1, 0, 2).contiguous()
        out = torch.zeros((self.P, self.ld))
        out[:, : 2 * self.L] = self.g.reshape(self.P, 2 * self.L)
        return out


# ------------------------------------------------------------------------------------------------ reference
def level_geometry(p32: Tensor, res32: Tensor):
    """floor / ceil corners (int64 [P, L, 3]) and the offsets (float32, exact) of `p32 * res32` formed in float32"""
    assert p32.dtype == torch.float32 and res32.dtype == torch.float32
    scaled = p32[:, None, :] * res32.view(1, -1, 1)
    f = torch.floor(scaled)
    return f.to(torch.int64), torch.ceil(scaled).to(torch.int64), scaled - f


def corner_slots(f: Tensor, c: Tensor, log2T: int) -> Tensor:
    """[P, L, 8] slots inside the level; corner k = (z, y, x) bits, 1 = ceil"""
    T = 1 << log2T
    xs, ys, zs = (f[..., 0], c[..., 0]), (f[..., 1] * PRIME_Y, c[..., 1] * PRIME_Y), (f[..., 2] * PRIME_Z, c[..., 2] * PRIME_Z)
    return torch.stack([(xs[k & 1] ^ ys[(k >> 1) & 1] ^ zs[k >> 2]) % T for k in range(8)], dim=-1)


def reference_scatter(p32: Tensor, res32: Tensor, log2T: int, g64: Tensor):
    """-> (grad64 [L * T, 2], A64 [L * T, 2], count [L * T]) for g64 [P, L, 2]"""
    T, L = 1 << log2T, res32.shape[0]
    f, c, o = level_geometry(p32, res32)
    o = o.double()
    w1 = (1.0 - o, o)
    slots = corner_slots(f, c, log2T) + (torch.arange(L) * T).view(1, L, 1)
    grad = torch.zeros((L * T, 2), dtype=torch.float64)
    A = torch.zeros((L * T, 2), dtype=torch.float64)
    count = torch.zeros(L * T, dtype=torch.int64)
    for k in range(8):
        w = w1[k & 1][..., 0] * w1[(k >> 1) & 1][..., 1] * w1[k >> 2][..., 2]  # [P, L]
        idx = slots[..., k].reshape(-1)
        grad.index_add_(0, idx, (w[..., None] * g64).reshape(-1, 2))
        A.index_add_(0, idx, (w[..., None] * g64.abs()).reshape(-1, 2))
        count.index_add_(0, idx, torch.ones_like(idx))
    return grad, A, count


# ------------------------------------------------------------------------------------------------ census
def patch_order(i: np.ndarray, N: int, S: int):
    """tn_patch_order: work item -> (ray, sample)"""
    per = 4 * S
    grp = i // per
    w = i - grp * per
    r0 = grp * 4
    nr = np.minimum(N - r0, 4)
    s = np.where(nr == 4, w >> 2, w // np.maximum(nr, 1))
    return r0 + (w - s * nr), s


def _cdiv(a, b):
    return -(-a // b)


def seg_plan(L: int, log2T: int, P: int) -> dict:
    slice_log2 = min(SLICE_LOG2, log2T)
    ns = 1 << (log2T - slice_log2)
    NB = _cdiv(P, BIN_THREADS)
    segc = 1024 if L * ns >= 1024 else max(64, min(1024, 8 * ns))
    segc = min(segc, NB)
    segc = _cdiv(NB, _cdiv(NB, segc))
    lg = 1
    while lg < L and NB * lg < 256 * 6:
        lg *= 2
    return dict(slice_log2=slice_log2, nslices=ns, NB=NB, segc=segc, chunks=_cdiv(NB, segc), level_groups=min(lg, L))


def bin_plan(L: int, log2T: int, P: int, res32: Tensor) -> dict:
    sp = seg_plan(L, log2T, P)
    ns, NB = sp["nslices"], sp["NB"]
    cap = ((16 * P + MAX_SLICES * 1032) // ns) & ~7
    chunk = []
    for l in range(L):
        r1 = float(np.ceil(float(res32[l]))) + 1.0
        T = float(1 << log2T)
        live = min(r1 ** 3, T)
        chunk.append(SPARSE_CHUNK if (r1 ** 3 < 0.5 * T or 8.0 * P > 16.0 * live) else DENSE_CHUNK)
    lg = 1
    while lg < L and (NB * lg < 256 * 6 or _cdiv(L, lg) * ns > BIN_MAX_COUNTERS):
        lg *= 2
    return dict(cap=cap, chunk=chunk, level_groups=min(lg, L))


def plan_replicas(L: int, log2T: int, P: int, res32: Tensor) -> list:
    """which levels the atomic path accumulates in dense replicas"""
    cap, T, used, out = SCRATCH_BYTES // 8, 1 << log2T, 0, []
    for l in range(L):
        r = float(res32[l])
        ok = False
        if 1.0 <= r <= 62.0:
            n = (int(np.ceil(r)) + 1) ** 3
            ok = n <= T and n <= 4 * P and used + n * REPLICAS <= cap
            if ok:
                used += n * REPLICAS
        if not ok:
            break
        out.append(True)
    return out + [False] * (L - len(out))


def census(case: Case) -> dict:
    L, log2T, P = case.L, case.log2T, case.P
    sp = seg_plan(L, log2T, P)
    bp = bin_plan(L, log2T, P, case.res)
    ns, NB, sl2 = sp["nslices"], sp["NB"], sp["slice_log2"]
    lanes = NB * BIN_THREADS
    i = np.arange(lanes, dtype=np.int64)
    live = i < P
    ray, s = patch_order(np.minimum(i, P - 1), case.N, case.S)
    order = torch.from_numpy(ray * case.S + s)
    f, c, o = level_geometry(case.p32[order], case.res)
    slots = corner_slots(f, c, log2T).numpy()  # [lanes, L, 8]
    f, onl = f.numpy(), (o == 0).numpy()
    wave_lane = i % 64
    runs, heads = [], []
    records = np.zeros((L, NB, ns), dtype=np.int64)
    for l in range(L):
        key = np.concatenate([f[:, l, :], onl[:, l, :].astype(np.int64)], axis=1)  # floor cell + which axes sit on the lattice
        head = np.ones(lanes, dtype=bool)
        head[1:] = (wave_lane[1:] == 0) | (key[1:] != key[:-1]).any(axis=1) | ~live[1:]
        hp = np.flatnonzero(head)
        length = np.diff(np.append(hp, lanes))
        keep = live[hp]
        runs.append(np.stack([hp[keep] // 64, hp[keep] % 64, length[keep]], axis=1))  # (wave, first lane, length)
        heads.append(head)
        tail = np.ones(lanes, dtype=bool)
        tail[:-1] = head[1:]
        emit = np.flatnonzero(live & tail)
        np.add.at(records[l], (np.repeat(emit // BIN_THREADS, 8), (slots[emit, l, :] >> sl2).reshape(-1)), 1)
    segc, chunks = sp["segc"], sp["chunks"]
    gw = np.full((L, ns, chunks), -1, dtype=np.int64)
    empty_first = empty_mid = empty_last = odd = 0
    for l in range(L):
        for b in range(ns):
            for ch in range(chunks):
                seg = records[l, ch * segc: min(NB, (ch + 1) * segc), b]
                total = int(((seg + 1) // 2).sum())
                if total == 0:
                    continue
                avg = 2 * total // len(seg)
                gw[l, b, ch] = 6 if avg >= 256 else (5 if avg >= 96 else 4)
                odd += int((seg % 2 == 1).sum())
                if len(seg) >= 3:
                    empty_first += int(seg[0] == 0)
                    empty_last += int(seg[-1] == 0)
                    empty_mid += int((seg[1:-1] == 0).any())
    raw = records.sum(axis=1)  # [L, ns]
    nfold = np.maximum(1, _cdiv(np.minimum(raw, bp["cap"]), np.asarray(bp["chunk"])[:, None]))
    return dict(seg=sp, bin=bp, runs=runs, heads=heads, records=records, gw_log2=gw, odd_segments=odd, empty_first=empty_first, empty_mid=empty_mid,
                empty_last=empty_last, raw=raw, overflow=raw > bp["cap"], nfold=nfold, replicas=plan_replicas(L, log2T, P, case.res),
                max_run=int(max(int(r[:, 2].max()) for r in runs)), lane_order=order)


def addends(case: Case, cen: dict, count: Tensor, path: str):
    """-> (R, F [L * T] float64) of the bound for path "2" (segmented), "1" (binned), "0" (atomics with replicas) or "nows" (no workspace)"""
    T, L = 1 << case.log2T, case.L
    if path in ("0", "nows"):
        return 0, count.double()
    if path == "2":
        return cen["max_run"], torch.full((L * T,), float(cen["seg"]["chunks"]), dtype=torch.float64)
    per_bucket = torch.from_numpy(cen["nfold"]).double()  # [L, ns]
    over = torch.from_numpy(cen["overflow"])
    slots = 1 << cen["seg"]["slice_log2"]
    F = per_bucket.repeat_interleave(slots, dim=1).reshape(-1)
    F = F + torch.where(over.repeat_interleave(slots, dim=1).reshape(-1), count.double() - 1.0, torch.zeros(L * T, dtype=torch.float64)).clamp_min(0)
    return cen["max_run"], F


def prefill(case: Case, A: Tensor, count: Tensor) -> Tensor:
    """float32 [L * T, 2]: non-zero in a seeded half of the slots (see the module docstring)"""
    n = A.shape[0]
    pick = torch.from_numpy(synth.uniform("sc_pick_" + case.name, (n,), 0.0, 1.0, seed=5)) < 0.5
    v = torch.from_numpy(synth.uniform("sc_pre_" + case.name, (n, 2), seed=5)).double()
    v = torch.where(v == 0, torch.ones_like(v), v)
    touched = A > 0
    scaled = torch.sign(v) * (1.0 + v.abs()) * A / count.clamp_min(1).double()[:, None]
    out = torch.where(touched, scaled, v) * pick[:, None]
    return out.float()


# ------------------------------------------------------------------------------------------------ builders
def _u(name, shape, lo=0.0, hi=1.0):
    return synth.uniform("sc_" + name, shape, lo, hi, seed=7).astype(np.float64)


def _p_of(o32: np.ndarray) -> np.ndarray:
    return (o32 + np.float32(2.0)) / np.float32(4.0)


def _cell_points(tag: str, res32: Tensor, cell0, n: int, span: float) -> np.ndarray:
    """n origins (float32) whose points lie in ONE cell of every level, inside level-0 cell `cell0`, off the lattice, each at its own offset"""
    res = res32.numpy()
    rmax = float(res[-1])
    for attempt in range(200):
        b = (np.asarray(cell0, dtype=np.float64) + _u(f"{tag}_b{attempt}", (3,), 0.1, 0.9)) / 16.0
        b = (np.floor(b * rmax) + 0.05) / rmax
        p = b[None, :] + _u(f"{tag}_v{attempt}", (n, 3)) * span / rmax
        o32 = (4.0 * p - 2.0).astype(np.float32)
        sc = _p_of(o32)[:, None, :] * res[None, :, None]
        fl = np.floor(sc)
        if (fl == fl[:1]).all() and (sc != fl).all() and (fl[0, 0] == np.asarray(cell0)).all() and len(np.unique(o32, axis=0)) == n:
            return o32
    raise AssertionError(f"no cell found for {tag}")


def _span(gname):
    return 0.9 if gname != "G16" else 0.03  # (non-integral growth: a finest cell straddles coarser lattice planes)


def _cell_of_run(tag: str, r: int):
    """level-0 cells of neighbouring runs differ by at least 2 in x: their cells differ on every level"""
    yz = np.floor(_u(f"{tag}_c{r}", (2,), 4.0, 12.0)).astype(np.int64)
    return (4 + 2 * (r % 4), int(yz[0]), int(yz[1]))


def _point_case(name, gname, o32: np.ndarray, marks=None) -> Case:
    N = o32.shape[0]
    e = torch.tensor([[0.5, 1.0]]).repeat(N, 1)
    return Case(name, gname, N, 1, torch.from_numpy(np.ascontiguousarray(o32, dtype=np.float32)), torch.zeros(N, 3), e, -1, marks=marks)


def _from_runs(name, gname, lengths) -> Case:
    res = grid_res(gname)
    parts = [_cell_points(f"{name}_{r}", res, _cell_of_run(name, r), n, _span(gname)) for r, n in enumerate(lengths)]
    return _point_case(name, gname, np.concatenate(parts, axis=0))


def runs_layout() -> list:
    """run lengths in lane order (see the issue list in RUN_LENGTHS / RUN_STARTS): 16 waves and 37 lanes"""
    w = [[15, 1, 15, 1, 15, 1, 12, 8],                 # starts at 15, 16, 31, 32, 47, 48; 60..67 cut by the wave boundary
         [2, 3, 4, 5, 8, 9, 16, 13],                   # (from lane 68) 16 lanes over the row boundary at 112
         [64], [63, 1], [17, 31, 16], [32, 32], [33, 31],
         [48, 12, 8],                                  # 508..515 cut by the block boundary
         [48, 12],                                     # (from lane 516) lanes 4..51: over 16, 32 and 48
         [1] * 64, [2] * 32, [3, 4] * 9 + [1],         # the maxlen ladder: 1, 2, 4
         [5, 6, 7, 8] * 2 + [5, 7]]                    # 8
    lengths = [n for row in w for n in row]
    extra = np.floor(_u("runs_extra", (64,), 1.0, 21.0)).astype(int).tolist()
    for n in extra:  # three more waves of seeded lengths 1..20
        if sum(lengths) + n > 1024:
            break
        lengths.append(n)
    lengths.append(1024 - sum(lengths))
    if lengths[-1] == 0:
        lengths.pop()
    return lengths + [20, 17]  # the partial block: the last run ends on the last live lane


def _lattice() -> Case:
    res = grid_res("G5")
    rows, marks = [], {}

    def add(tag, o):
        marks[tag] = len(rows)
        rows.extend(np.asarray(o, dtype=np.float32).reshape(-1, 3))

    add("sel0_wave", np.tile([1e30, 0.0, 0.0], (64, 1)))  # wave 0: 64 selector-0 points (p = 0: every level's slot hash(0, 0, 0), weight 1)
    d = 4.0 * 0.3 / 256.0  # 0.3 of a finest cell, in origin units
    for k, (tag, on) in enumerate((("on1", (1, 0, 0)), ("on2", (1, 1, 0)), ("on3", (1, 1, 1)))):
        base = np.array([-0.75 + 0.5 * k, 0.25, -0.5])  # multiples of 1/4: p * 16 integral
        off_lattice = base + d
        add(tag, np.where(np.array(on) == 1, base, off_lattice))
        add(tag + "_off", off_lattice)  # same floor cell on every level, no axis on the lattice: must not merge
    live = _cell_points("lat_live", res, (5, 9, 6), 2, 0.9)
    add("live_a", live[0])
    add("sel0_single", [1e30, 0.0, 0.0])
    add("live_b", live[1])
    same = np.tile([0.5, -0.25 + d, 0.75 + d], (3, 1))  # three points on the plane x: one cell, the same flag -> one run
    same[:, 1:] += np.array([[0.0, 0.0], [d / 3, d / 2], [d / 2, d / 3]])
    add("on_run3", same)
    fill = 128 - len(rows)
    add("fill", np.concatenate([_cell_points(f"lat_fill{r}", res, _cell_of_run("lat_fill", r), 1, 0.9) for r in range(fill)]))
    add("on_wave", np.tile([0.25, -0.5, 0.5], (64, 1)))  # wave 2: 64 points on one lattice point of level 0
    add("tail", np.concatenate([_cell_points(f"lat_tail{r}", res, _cell_of_run("lat_tail", r), 1, 0.9) for r in range(8)]))
    return _point_case("lattice", "G5", np.stack(rows), marks)


def _hot_slot(name, gname, P, one_cell=False) -> Case:
    res = grid_res(gname)
    if one_cell:
        return _point_case(name, gname, _cell_points(name, res, (6, 9, 5), P, _span(gname)))
    a = _cell_points(name + "_a", res, (5, 6, 10), P // 2, _span(gname))
    b = _cell_points(name + "_b", res, (9, 7, 4), P // 2, _span(gname))
    return _point_case(name, gname, np.stack([a, b], axis=1).reshape(P, 3))


def _spread(name, gname, P, packed_blocks=(), run=None) -> Case:
    res = grid_res(gname)
    o = synth.uniform("sc_spread_" + name, (P, 3), -3.0, 3.0, seed=7)
    if run is not None:  # every wave: runs of `run` lanes, each in a cell of its own
        o = o.copy()
        r = 0
        for w0 in range(0, P, 64):
            at = w0
            for n in run:
                n = min(n, P - at)
                if n <= 0:
                    break
                o[at:at + n] = _cell_points(f"{name}_{r}", res, _cell_of_run(name, r), n, _span(gname))
                at += n
                r += 1
    for b in packed_blocks:  # a bin block whose samples share one cell: a handful of records, most of its segments empty
        lo, hi = b * BIN_THREADS, min(P, (b + 1) * BIN_THREADS)
        o = o.copy()
        o[lo:hi] = _cell_points(f"{name}_pack{b}", res, _cell_of_run(name, b), hi - lo, _span(gname))
    return _point_case(name, gname, o)


def _odd(name, P) -> Case:
    """x between lattice planes 4095 and 4096 of the fine level of G8k: the two x corners of every sample fall into different buckets"""
    rfine = float(grid_res("G8k")[-1])
    assert rfine >= 4097
    p = np.concatenate([(4095.0 + _u(name + "_x", (P, 1), 0.05, 0.95)) / rfine, _u(name + "_yz", (P, 2), 0.27, 0.73)], axis=1)
    return _point_case(name, "G8k", (4.0 * p - 2.0).astype(np.float32))


def positions64(c: Case) -> Tensor:
    """the unit-cube positions formed in float64 from the same float32 inputs: what float64 autograd of the oracle differentiates"""
    e = c.e_bins.double()
    p, _ = orc.unit_cube_positions(orc.Samples(s_bins=e, e_bins=e).positions(c.origins.double(), c.directions.double()))
    return p.reshape(-1, 3)


def cells_agree(c: Case) -> bool:
    """d position is a sum of cell-wise constant slopes: a sample that float32 and float64 put on different sides of a lattice plane (its
    position or p * res rounds across it) makes the float64 derivative that of ANOTHER cell.  A ray case keeps such samples out: a condition on
    the inputs, checked without a GPU."""
    f32, c32, _ = level_geometry(c.p32, c.res)
    s64 = positions64(c)[:, None, :] * c.res.double().view(1, -1, 1)
    return bool((torch.floor(s64).long() == f32).all()) and bool((torch.ceil(s64).long() == c32).all())


def _rays(name, gname, N, S, ld) -> Case:
    s = orc.spaced_bins(N, S, None)
    e = orc.s_to_euclidean(s, torch.ones(N, 1) * 0.05, torch.ones(N, 1) * 1000.0).contiguous()
    for seed in range(11, 75):  # the first seed of synth_rays_simple whose samples float32 and float64 place in the same cells
        r = synth.synth_rays_simple(N, seed)
        c = Case(name, gname, N, S, torch.from_numpy(r["origins"]), torch.from_numpy(r["directions"]), e, ld, want_dpos=True, marks={"seed": seed})
        if cells_agree(c):
            return c
    raise AssertionError(f"no ray seed for {name}")


POINT_CASES = {
    "runs_G5": lambda: _from_runs("runs_G5", "G5", runs_layout()),
    "runs_G16": lambda: _from_runs("runs_G16", "G16", runs_layout()),
    "lattice": _lattice,
    "hot_slot_G5": lambda: _hot_slot("hot_slot_G5", "G5", 3 * 512),
    "hot_slot_G20": lambda: _hot_slot("hot_slot_G20", "G20", 8192),
    "one_cell_G5": lambda: _hot_slot("one_cell_G5", "G5", 3 * 512, one_cell=True),
    "spread_G5": lambda: _spread("spread_G5", "G5", 33000),
    "spread_G16": lambda: _spread("spread_G16", "G16", 5000, packed_blocks=(0, 4, 9)),
    "odd_G8k": lambda: _odd("odd_G8k", 2 * 512 + 200),
    "spread_runs_G5": lambda: _spread("spread_runs_G5", "G5", 3 * 512 + 100, run=(22, 21, 21)),
}
RAY_SHAPES = ((8, 16), (8, 24), (7, 16))
RAY_CASES = {}
for _N, _S in RAY_SHAPES:
    for _tag, _g, _ld in (("G5_rows", "G5", 16), ("G5_levels", "G5", -1), ("G16_rows", "G16", 32)):
        RAY_CASES[f"rays_{_N}x{_S}_{_tag}"] = functools.partial(_rays, f"rays_{_N}x{_S}_{_tag}", _g, _N, _S, _ld)
ALL_CASES = {**POINT_CASES, **RAY_CASES}


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    return ALL_CASES[name]()


@functools.lru_cache(maxsize=None)
def case_census(name: str) -> dict:
    return census(case(name))


@functools.lru_cache(maxsize=None)
def case_reference(name: str):
    c = case(name)
    return reference_scatter(c.p32, c.res, c.log2T, c.g.double())
