"""Edge-weighted neighbour sampling without a GPU: the contract of include/bot_gnn.h (csrc/sampling_weighted.hip) restated in
numpy — per-row exact quantisation, the 96-bit Philox draw, successive sampling without replacement — with statistical checks of
the restatement, and the new entry points exported and validating their arguments.  tests/test_weighted_sampling_gpu.py holds
the kernels to this restatement bit for bit."""
import ctypes
import inspect
from itertools import combinations

import numpy as np
import pytest

from tests.test_sampling_host import M64, philox4x32_10


def quantise_row(w) -> np.ndarray:
    """q_i = floor(w_i * 2^(33 - e)), w_max = m * 2^e with m in [0.5, 1): uint64, exact (a power-of-two scale in fp64)."""
    w = np.asarray(w, dtype=np.float32)
    if w.size and not (np.all(w >= 0) and np.all(np.isfinite(w))):
        raise ValueError("a weight is negative, NaN or infinite")
    w = w.astype(np.float64)
    if w.size == 0 or w.max() <= 0:
        return np.zeros(w.size, dtype=np.uint64)
    _, e = np.frexp(w.max())
    return np.floor(np.ldexp(w, 33 - int(e))).astype(np.uint64)


def philox_words(seed: int, v: int, ms) -> np.ndarray:
    """Words x0..x2 of Philox4x32-10(seed, v << 32 | m) per round m: uint32 [len(ms), 3]."""
    ctr = (np.uint64(v) << np.uint64(32)) | np.asarray(ms, dtype=np.uint64)
    return philox4x32_10(seed & M64, ctr)[:, :3]


def draw(x, Q: int) -> int:
    """t = floor(r * Q / 2^96), r = x0 * 2^64 + x1 * 2^32 + x2, as (hi64 * Q + floor(x2 * Q / 2^32)) >> 64."""
    hi = (int(x[0]) << 32) | int(x[1])
    return (hi * Q + ((int(x[2]) * Q) >> 32)) >> 64


def weighted_sample_row(seed: int, v: int, q: np.ndarray, k: int) -> np.ndarray:
    """Offsets (ascending) the weighted sampler takes from row v with quantised weights q."""
    positive = np.nonzero(q)[0]
    if k < 0 or positive.size <= k:
        return positive.astype(np.int64)
    x = philox_words(seed, v, np.arange(k))
    left = q.copy()
    q_rem = int(q.sum(dtype=np.uint64))
    taken = []
    for m in range(k):
        t = draw(x[m], q_rem)
        assert t < q_rem
        i = int(np.searchsorted(np.cumsum(left, dtype=np.uint64), np.uint64(t), side="right"))   # smallest i with C(i) > t
        assert left[i] > 0
        taken.append(i)
        q_rem -= int(left[i])
        left[i] = 0
    return np.sort(np.array(taken, dtype=np.int64))


def weighted_reference(indptr, eid, w, seeds, k: int, seed: int):
    """(offsets int64 [n+1], CSC positions) — the contract of bot_sample_neighbors_weighted_i32 (w in edge-id order)."""
    rows = []
    for v in seeds:
        base, end = int(indptr[v]), int(indptr[v + 1])
        rows.append(base + weighted_sample_row(seed, int(v), quantise_row(w[eid[base:end]]), k))
    offsets = np.zeros(len(seeds) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(r) for r in rows])
    return offsets, (np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64))


def test_quantisation_is_exact_and_scale_free():
    q = quantise_row([1, 2, 3, 4])
    assert q.tolist() == [2 ** 30, 2 ** 31, 3 * 2 ** 30, 2 ** 32]
    rng = np.random.default_rng(0)
    w = rng.random(1000, dtype=np.float32) + np.float32(1e-3)
    q = quantise_row(w)
    assert 2 ** 32 <= int(q.max()) < 2 ** 33
    for s in (-100, -20, 7, 60, 100):                     # every weight stays a normal fp32
        ws = np.ldexp(w, s).astype(np.float32)
        assert np.all(np.isfinite(ws)) and ws.min() >= np.finfo(np.float32).tiny
        assert np.array_equal(quantise_row(ws), q), s
    assert quantise_row([1.0, 1e-12, 0.0]).tolist() == [2 ** 33 // 2, 0, 0]   # below ~2^-33 of the row's largest: zero
    assert quantise_row([0.0, -0.0]).tolist() == [0, 0]
    sub = np.array([1e-45, 3e-42, 1e-40], dtype=np.float32)                      # subnormals: still 2^32 <= q_max < 2^33
    assert 2 ** 32 <= int(quantise_row(sub).max()) < 2 ** 33
    big = np.array([3e38, 1e38, 1.0], dtype=np.float32)
    assert quantise_row(big)[2] == 0 and int(quantise_row(big).sum(dtype=np.uint64)) < 2 ** 64
    for bad in ([1.0, -1.0], [np.nan], [np.inf, 1.0], [-np.inf]):
        with pytest.raises(ValueError):
            quantise_row(bad)


def test_draw_is_exact_and_below_the_total():
    x = philox_words(99, 5, np.arange(500))
    for Q in (1, 3, 2 ** 33 - 1, 10 ** 15 + 7, 2 ** 64 - 1):
        for m in range(500):
            r = (int(x[m, 0]) << 64) | (int(x[m, 1]) << 32) | int(x[m, 2])
            t = draw(x[m], Q)
            assert t == (r * Q) >> 96 and 0 <= t < Q


def test_first_round_pick_is_proportional_to_q():
    """k = 1 over 40000 row ids: the pick histogram against n q_i / Q (chi-square, 9 degrees of freedom: 99.9th percentile 27.9)."""
    w = np.array([0.5, 1, 2, 3, 0.25, 4, 1.5, 6, 0.75, 5], dtype=np.float32)
    q = quantise_row(w)
    n, seed = 40000, 31337
    x = philox4x32_10(seed, np.arange(n, dtype=np.uint64) << np.uint64(32))
    cs = np.cumsum(q, dtype=np.uint64)
    Q = int(cs[-1])
    hist = np.zeros(w.size)
    for v in range(n):
        t = draw(x[v], Q)
        i = int(np.searchsorted(cs, np.uint64(t), side="right"))
        hist[i] += 1
        if v < 300:                                         # the row sampler takes the same edge
            assert weighted_sample_row(seed, v, q, 1).tolist() == [i]
    exp = n * q.astype(np.float64) / Q
    chi2 = float(((hist - exp) ** 2 / exp).sum())
    assert chi2 < 27.9, chi2


def test_pair_inclusion_matches_successive_sampling():
    """k = 2 on weights (1, 2, 3, 4): P({i, j}) = p_i p_j / (1 - p_i) + p_j p_i / (1 - p_j); 12000 rows, 5 degrees of freedom
    (99.9th percentile 20.5)."""
    w = np.array([1, 2, 3, 4], dtype=np.float32)
    q = quantise_row(w)
    p = w.astype(np.float64) / w.sum()
    n = 12000
    pairs = list(combinations(range(4), 2))
    hist = dict.fromkeys(pairs, 0)
    for v in range(n):
        r = weighted_sample_row(2718, v, q, 2)
        assert len(r) == 2 and r[0] < r[1]
        hist[(int(r[0]), int(r[1]))] += 1
    exp = {(i, j): n * (p[i] * p[j] / (1 - p[i]) + p[j] * p[i] / (1 - p[j])) for i, j in pairs}
    assert abs(sum(exp.values()) - n) < 1e-6
    chi2 = sum((hist[c] - exp[c]) ** 2 / exp[c] for c in pairs)
    assert chi2 < 20.5, (chi2, hist, exp)


def test_zero_weights_are_never_taken_and_short_rows_return_their_positive_set():
    rng = np.random.default_rng(3)
    w = rng.random(40, dtype=np.float32)
    w[rng.permutation(40)[:15]] = 0
    w[3] = np.float32(1e-12)                             # quantises to zero next to weights of order 1
    q = quantise_row(w)
    assert q[3] == 0
    zero = set(np.nonzero(q == 0)[0].tolist())
    n_pos = 40 - len(zero)
    for v in range(400):
        r = weighted_sample_row(11, v, q, 6)
        assert len(r) == 6 and len(np.unique(r)) == 6 and not (set(r.tolist()) & zero)
    for k in (n_pos, n_pos + 1, 1024, -1):
        assert np.array_equal(weighted_sample_row(11, 0, q, k), np.nonzero(q)[0]), k
    assert weighted_sample_row(11, 0, quantise_row(np.zeros(9, dtype=np.float32)), 4).size == 0
    assert weighted_sample_row(11, 0, quantise_row(np.zeros(0, dtype=np.float32)), 4).size == 0
    # without replacement: k = n_pos - 1 leaves exactly one positive edge out
    r = weighted_sample_row(12, 1, q, n_pos - 1)
    assert len(np.unique(r)) == n_pos - 1 and set(r.tolist()) < set(np.nonzero(q)[0].tolist())


def test_scaling_a_row_by_a_power_of_two_keeps_the_picks():
    rng = np.random.default_rng(8)
    w = (rng.random(300, dtype=np.float32) * 10).astype(np.float32)
    w[::7] = 0
    q = quantise_row(w)
    for s in (-60, -3, 1, 40):
        ws = np.ldexp(w, s).astype(np.float32)
        for v in range(30):
            assert np.array_equal(weighted_sample_row(5, v, quantise_row(ws), 8), weighted_sample_row(5, v, q, 8)), (s, v)


def test_weighted_symbols_are_exported_and_validate_arguments():
    from bot_amd import _C
    lib = _C._lib
    for name in ("bot_sample_weights_prepare_f32", "bot_sample_neighbors_weighted_count_i32", "bot_sample_neighbors_weighted_i32"):
        assert name in _C.EXPORTED
        assert hasattr(lib, name)
    assert lib.bot_abi_version() == 19
    buf = (ctypes.c_int32 * 16)()
    off = (ctypes.c_int64 * 16)()
    p, o = ctypes.addressof(buf), ctypes.addressof(off)
    # NULL pointers -> -1
    assert lib.bot_sample_weights_prepare_f32(None, p, 4, 8, p, o, p, p, None) == -1
    assert lib.bot_sample_weights_prepare_f32(p, p, 4, 8, p, o, p, None, None) == -1
    assert lib.bot_sample_weights_prepare_f32(p, None, 4, 8, p, o, p, p, None) == -1
    assert lib.bot_sample_weights_prepare_f32(p, p, 4, 8, p, None, p, p, None) == -1
    assert lib.bot_sample_weights_prepare_f32(p, p, 4, 8, p, o, None, p, None) == -1
    assert lib.bot_sample_neighbors_weighted_count_i32(None, 4, p, 2, 3, p, None) == -1
    assert lib.bot_sample_neighbors_weighted_count_i32(p, 4, None, 2, 3, p, None) == -1
    assert lib.bot_sample_neighbors_weighted_count_i32(p, 4, p, 2, 3, None, None) == -1
    assert lib.bot_sample_neighbors_weighted_i32(None, o, p, 4, p, 2, 3, 7, o, p, None) == -1
    assert lib.bot_sample_neighbors_weighted_i32(p, None, p, 4, p, 2, 3, 7, o, p, None) == -1
    assert lib.bot_sample_neighbors_weighted_i32(p, o, None, 4, p, 2, 3, 7, o, p, None) == -1
    assert lib.bot_sample_neighbors_weighted_i32(p, o, p, 4, p, 2, 3, 7, None, p, None) == -1
    # nonsense sizes and k > 1024 -> -2
    assert lib.bot_sample_weights_prepare_f32(p, p, -1, 8, p, o, p, p, None) == -2
    assert lib.bot_sample_weights_prepare_f32(p, p, 4, -8, p, o, p, p, None) == -2
    assert lib.bot_sample_weights_prepare_f32(p, p, 4, 2 ** 31, p, o, p, p, None) == -2
    assert lib.bot_sample_neighbors_weighted_count_i32(p, -1, p, 2, 3, p, None) == -2
    assert lib.bot_sample_neighbors_weighted_count_i32(p, 4, p, -2, 3, p, None) == -2
    assert lib.bot_sample_neighbors_weighted_count_i32(p, 4, p, 2, 1025, p, None) == -2
    assert lib.bot_sample_neighbors_weighted_i32(p, o, p, 4, p, 2, 1025, 7, o, p, None) == -2
    assert lib.bot_sample_neighbors_weighted_i32(p, o, p, 4, p, -2, 3, 7, o, p, None) == -2
    # no seeds (no rows) -> 0, nothing launched, so no GPU is needed
    assert lib.bot_sample_weights_prepare_f32(p, None, 0, 0, None, None, None, p, None) == 0
    assert lib.bot_sample_neighbors_weighted_count_i32(p, 4, None, 0, 3, None, None) == 0
    assert lib.bot_sample_neighbors_weighted_i32(p, None, p, 4, None, 0, 3, 7, None, None, None) == 0


def test_weighted_sampler_surface_without_gpu():
    from bot_amd import sampling, workloads
    s = sampling.MultiLayerNeighborSampler([8], prob="w")
    assert s.fanouts == [8] and s.prob == "w"
    assert sampling.MultiLayerNeighborSampler([8, 4]).prob is None
    with pytest.raises(NotImplementedError):
        sampling.MultiLayerNeighborSampler([8], replace=True, prob="w")
    with pytest.raises(TypeError):
        sampling.MultiLayerNeighborSampler([8], prob=3)
    assert "prob" in inspect.signature(sampling.sample_block).parameters
    assert "prob" in inspect.signature(workloads.build_sampled).parameters
