"""Neighbour sampling without a GPU: the new entry points are exported and validate their arguments, and the sampler contract
(csrc/sampling.hip: Floyd's algorithm over Philox4x32-10 draws), restated here in numpy, is uniform and exactly without
replacement.  tests/test_sampling_gpu.py holds the kernels to this restatement bit for bit."""
import ctypes

import numpy as np
import pytest

M64 = (1 << 64) - 1


def philox4x32_10(seed: int, ctr: np.ndarray) -> np.ndarray:
    """Philox4x32-10 (csrc/common.h Philox::gen) of 64-bit counters `ctr` (uint64 array) under the 64-bit key `seed`:
    uint32 [n, 4]."""
    ctr = np.asarray(ctr, dtype=np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    c0, c1 = ctr & m32, ctr >> np.uint64(32)
    c2 = np.zeros_like(c0)
    c3 = np.zeros_like(c0)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)
        n1 = p1 & m32
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        n3 = p0 & m32
        c0, c1, c2, c3 = n0, n1, n2, n3
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def floyd_draws(seed: int, v: int, js: np.ndarray) -> np.ndarray:
    """t_j = umulhi64(r, j + 1), r = the first 64 bits of Philox(seed, v << 32 | j): uniform on {0..j}, bias < 2^-32."""
    js = np.asarray(js, dtype=np.uint64)
    r = philox4x32_10(seed & M64, (np.uint64(v) << np.uint64(32)) | js).astype(np.uint64)
    hi, lo, m = r[:, 0], r[:, 1], js + np.uint64(1)
    return ((hi * m + ((lo * m) >> np.uint64(32))) >> np.uint64(32)).astype(np.int64)   # < 2^64 for m < 2^32: no overflow


def sample_row(seed: int, v: int, deg: int, k: int) -> np.ndarray:
    """Offsets (0..deg-1, ascending) of the in-edges the sampler takes from row v."""
    if k < 0 or deg <= k:
        return np.arange(deg, dtype=np.int64)
    first = deg - k
    t = floyd_draws(seed, v, np.arange(first, deg))
    taken = set()
    for m in range(k):
        taken.add(first + m if int(t[m]) in taken else int(t[m]))
    return np.array(sorted(taken), dtype=np.int64)


def sample_reference(indptr: np.ndarray, seeds: np.ndarray, k: int, seed: int):
    """(offsets int64 [n+1], CSC positions) — the contract of bot_sample_neighbors_i32."""
    rows = [indptr[v] + sample_row(seed, int(v), int(indptr[v + 1] - indptr[v]), k) for v in seeds]
    offsets = np.zeros(len(seeds) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(r) for r in rows])
    return offsets, (np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64))


def test_philox_matches_the_published_known_answer():
    # Random123's kat_vectors: philox4x32-10 of counter 0 / key 0 is 6627e8d5 e169c58d bc57ac4c 9b00dbd8 (only counter words 0-1 and
    # the key are free in this form)
    assert [hex(int(x)) for x in philox4x32_10(0, np.array([0], dtype=np.uint64))[0]] == ["0x6627e8d5", "0xe169c58d", "0xbc57ac4c", "0x9b00dbd8"]


def test_draw_is_in_range_and_rows_are_without_replacement():
    for deg, k in ((50, 8), (9, 8), (100000, 100), (33, 32), (2, 1)):
        for v in range(20):
            r = sample_row(123 + v, v, deg, k)
            assert len(r) == min(deg, k) and len(np.unique(r)) == len(r)
            assert np.all(np.diff(r) > 0) and r.min() >= 0 and r.max() < deg
    for deg, k in ((0, 8), (5, 8), (8, 8), (7, -1), (1000, -1)):
        assert np.array_equal(sample_row(9, 3, deg, k), np.arange(deg))
    t = floyd_draws(77, 5, np.arange(0, 4096))
    assert np.all(t >= 0) and np.all(t <= np.arange(0, 4096))


def test_inclusion_frequencies_are_uniform():
    """deg 50, k 8 over 5000 rows (distinct v, one seed): each of the 50 edges is taken with probability 8/50; the counts pass a
    chi-square bound (49 degrees of freedom: 99.9th percentile 85.4), and so does the first-position count (which edge comes first)."""
    deg, k, n = 50, 8, 5000
    counts = np.zeros(deg)
    first = np.zeros(deg)
    for v in range(n):
        r = sample_row(2024, v, deg, k)
        counts[r] += 1
        first[r[0]] += 1
    exp = n * k / deg
    # inclusion indicators of one row are negatively correlated (exactly k of deg): the variance of a count is n p (1 - p) (deg-1)/(deg-1)
    chi2 = float(((counts - exp) ** 2 / (exp * (1 - k / deg))).sum())
    assert chi2 < 85.4, chi2
    # the smallest taken offset j has P = C(deg-1-j, k-1) / C(deg, k): compare the first-position histogram against it
    from math import comb
    p = np.array([comb(deg - 1 - j, k - 1) / comb(deg, k) for j in range(deg)])
    assert abs(p.sum() - 1) < 1e-12
    keep = p * n >= 5
    e = p[keep] * n
    o = first[keep]
    chi2f = float(((o - e) ** 2 / e).sum()) + float(((first[~keep].sum() - p[~keep].sum() * n) ** 2) / max(p[~keep].sum() * n, 1e-9))
    assert chi2f < 85.4, chi2f


def test_pairwise_inclusion_is_uniform():
    """Without replacement, every PAIR of edges is taken together with probability k(k-1) / (deg(deg-1)): deg 10, k 3, 6000 rows."""
    deg, k, n = 10, 3, 6000
    pair = np.zeros((deg, deg))
    for v in range(n):
        r = sample_row(5, v, deg, k)
        for a in r:
            for b in r:
                if a < b:
                    pair[a, b] += 1
    iu = np.triu_indices(deg, 1)
    exp = n * k * (k - 1) / (deg * (deg - 1))
    chi2 = float(((pair[iu] - exp) ** 2 / exp).sum())
    assert chi2 < 80.1, chi2       # 44 degrees of freedom, 99.9th percentile


def test_sampling_symbols_are_exported_and_validate_arguments():
    from bot_amd import _C
    lib = _C._lib
    for name in ("bot_sample_neighbors_count_i32", "bot_sample_neighbors_i32", "bot_block_tiles", "bot_block_mark_i32", "bot_block_relabel_i32"):
        assert name in _C.EXPORTED
        assert hasattr(lib, name)
    assert lib.bot_abi_version() == 19
    buf = (ctypes.c_int32 * 16)()
    off = (ctypes.c_int64 * 16)()
    p, o = ctypes.addressof(buf), ctypes.addressof(off)
    # NULL pointers -> -1
    assert lib.bot_sample_neighbors_count_i32(None, 4, p, 2, 3, p, None) == -1
    assert lib.bot_sample_neighbors_count_i32(p, 4, None, 2, 3, p, None) == -1
    assert lib.bot_sample_neighbors_i32(None, 4, p, 2, 3, 7, o, p, None) == -1
    assert lib.bot_sample_neighbors_i32(p, 4, p, 2, 3, 7, None, p, None) == -1
    assert lib.bot_block_mark_i32(p, 2, p, p, 3, None, 4, o, o, None) == -1
    assert lib.bot_block_mark_i32(None, 2, p, p, 3, p, 4, o, o, None) == -1
    assert lib.bot_block_relabel_i32(p, 2, p, p, p, 3, None, 4, o, 3, p, p, p, None) == -1
    assert lib.bot_block_relabel_i32(p, 2, p, None, p, 3, p, 4, o, 3, p, p, p, None) == -1
    # nonsense sizes -> -2
    assert lib.bot_sample_neighbors_count_i32(p, -1, p, 2, 3, p, None) == -2
    assert lib.bot_sample_neighbors_count_i32(p, 4, p, -2, 3, p, None) == -2
    assert lib.bot_sample_neighbors_i32(p, 4, p, 2, 5000, 7, o, p, None) == -2      # fan-out beyond the without-replacement path
    assert lib.bot_block_mark_i32(p, 5, p, p, 3, p, 4, o, o, None) == -2            # more seeds than nodes
    assert lib.bot_block_mark_i32(p, 2, p, p, -3, p, 4, o, o, None) == -2
    assert lib.bot_block_relabel_i32(p, 3, p, p, p, 3, p, 4, o, 2, p, p, p, None) == -2   # n_src below n_seeds
    assert lib.bot_block_relabel_i32(p, 2, p, p, p, 3, p, 4, o, 5, p, p, p, None) == -2   # n_src beyond n_nodes
    assert lib.bot_block_tiles(-1) == 0 and lib.bot_block_tiles(1) == 1
    # an empty seed list is a no-op: nothing launched, so no GPU is needed
    assert lib.bot_sample_neighbors_count_i32(p, 4, None, 0, 3, None, None) == 0
    assert lib.bot_sample_neighbors_i32(p, 4, None, 0, 3, 7, None, None, None) == 0
    assert lib.bot_block_mark_i32(None, 0, None, None, 0, p, 4, None, o, None) == 0
    assert lib.bot_block_relabel_i32(None, 0, None, None, None, 0, p, 4, None, 0, None, None, None, None) == 0


def test_sampler_surface_without_gpu():
    from bot_amd import sampling
    with pytest.raises(NotImplementedError):
        sampling.MultiLayerNeighborSampler([8, 8], replace=True)
    assert sampling.MultiLayerFullNeighborSampler(3).fanouts == [-1, -1, -1]
    assert sampling.MultiLayerNeighborSampler([8, 8, 4]).fanouts == [8, 8, 4]
