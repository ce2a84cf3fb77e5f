"""ROC-AUC as a Mann-Whitney count restated in numpy (the contract of bot_rocauc_f32, include/bot_gnn.h, and of
`bot_amd.metrics.rocauc_counts`), and the case generator shared by tests/test_metrics_host.py (where the restatement is itself held
to scikit-learn) and tests/test_metrics_gpu.py (which holds the kernels to it integer for integer)."""
import numpy as np

FAMILIES = ("continuous", "levels2", "levels7", "levels300", "equal", "special", "large")


def counts_reference(pred, labels, groups=None, n_groups=1):
    """int64 [G, T, 3] = (n_pos, n_neg, 2U) per group and task, and the number of NaN scores among the counted entries.
    pred float32 [n, T]; labels [n, T], 1 positive, 0 negative, anything else (a float NaN too) ignored; groups [n] integers,
    g in [0, G) or anything else = the row is excluded.  Stable argsort of score + 0.0 as float32, tie groups,
    sum pos_g * (2 * neg_below_g + neg_g) in int64."""
    pred = np.asarray(pred, dtype=np.float32)
    labels = np.asarray(labels)
    n, T = pred.shape
    G = int(n_groups)
    g = np.zeros(n, dtype=np.int64) if groups is None else np.asarray(groups).astype(np.int64)
    out = np.zeros((G, T, 3), dtype=np.int64)
    nans = 0
    with np.errstate(invalid="ignore"):
        is_pos, is_neg = labels == 1, labels == 0
    for t in range(T):
        s = (pred[:, t] + np.float32(0.0)).astype(np.float32)
        for k in range(G):
            rows = (g == k) & (is_pos[:, t] | is_neg[:, t])
            nan = rows & np.isnan(s)
            nans += int(nan.sum())
            rows &= ~nan
            sk, pk = s[rows], is_pos[rows, t].astype(np.int64)
            order = np.argsort(sk, kind="stable")
            sk, pk = sk[order], pk[order]
            nk = 1 - pk
            out[k, t, 0], out[k, t, 1] = pk.sum(), nk.sum()
            if len(sk) == 0:
                continue
            first = np.flatnonzero(np.concatenate([[True], sk[1:] != sk[:-1]]))      # -0.0 == +0.0; denormals differ
            pos_r, neg_r = np.add.reduceat(pk, first), np.add.reduceat(nk, first)
            below = np.cumsum(neg_r) - neg_r
            out[k, t, 2] = int((pos_r * (2 * below + neg_r)).sum())
    return out, nans


def mean_auc_reference(counts):
    """float64 [G]: the mean of 2U / (2 n_pos n_neg) over the tasks with both classes; NaN where there is none."""
    counts = np.asarray(counts)
    out = np.full(counts.shape[0], np.nan)
    for k in range(counts.shape[0]):
        p, q, u2 = (counts[k, :, i].astype(np.float64) for i in range(3))
        ok = (p > 0) & (q > 0)
        if ok.any():
            out[k] = (u2[ok] / (2.0 * p[ok] * q[ok])).mean()
    return out


def scores(family, n, T, rng):
    """float32 [n, T] of one score family: continuous; 2 / 7 / 300 distinct levels; all equal; "special" (+-0.0, +-inf, denormals
    beside ordinary values); "large" (logits of magnitude 125)."""
    if family == "continuous":
        x = rng.standard_normal((n, T))
    elif family.startswith("levels"):
        x = rng.integers(0, int(family[6:]), (n, T)) * 0.37 - 1.0
    elif family == "equal":
        x = np.full((n, T), 0.25)
    elif family == "special":
        pool = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 3e-39, -3e-39, 1.1754944e-38, 1.0, -1.0, 2.5], dtype=np.float32)
        return pool[rng.integers(0, len(pool), (n, T))]
    elif family == "large":
        x = rng.standard_normal((n, T)) * 125.0
    else:
        raise ValueError(family)
    return x.astype(np.float32)


def case(family, n, T, G, seed, unlabelled=0.05, excluded=0.1):
    """(pred float32 [n, T], labels int8 [n, T] with -1 = not labelled, groups int8 [n] or None): task 0 keeps both classes where
    n allows; with T >= 3 task 1 holds one class only; with G = 3 the rows are cut about 54 / 18 / 28 % and some are excluded."""
    rng = np.random.default_rng(seed)
    pred = scores(family, n, T, rng)
    labels = (rng.random((n, T)) < 0.4).astype(np.int8)
    labels[rng.random((n, T)) < unlabelled] = -1
    if T >= 3:
        labels[:, 1] = 1
    groups = None
    if G > 1:
        u = rng.random(n)
        groups = np.where(u < 0.54, 0, np.where(u < 0.72, 1, 2)).astype(np.int8) % G
        groups[rng.random(n) < excluded] = -1
    return pred, labels, groups
