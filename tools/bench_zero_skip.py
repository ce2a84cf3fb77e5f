#!/usr/bin/env python3
"""The zero-weight skip of the hidden layer's sparse sweeps, timed in isolation (csrc/spmm.hip, `_C.spmm_set_zero_skip`).

S-arxiv at scale 1.0, H = 3, D = 250: the forward sweep (`_C.spmm` on the CSC, weights in position order) and the halves form of the
fused backward (`_C.spmm_dot_halves` on the CSR through csr2csc), with attention weights from `_C.gat_attn_fwd` at attention dropout
0.0 (no exact zeros: what the skip costs) and 0.1 (10 % of the (edge, head) weights are 0.f: what it saves).  The switch alternates
off / on in ONE process, REPEATS times; every repeat is the median of ITERS launches between HIP events.  One JSON line per
(sweep, dropout) case:

    python tools/bench_zero_skip.py [out.jsonl]        default profiles/bench_zero_skip.jsonl
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bot_amd  # noqa: E402,F401
from bot_amd import _C, synth  # noqa: E402

H, D = 3, 250
DEV = "cuda"
REPEATS, ITERS, WARM = 12, 20, 3


def median_ms(fn):
    for _ in range(WARM):
        fn()
    evs = []
    for _ in range(ITERS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        evs.append((e0, e1))
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in evs)
    return ts[len(ts) // 2]


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bench_zero_skip.jsonl")
    ds = synth.make_dataset("arxiv", device="cpu", seed=0, scale=1.0)
    g = ds.graph.to(DEV)
    g.create_formats_()
    n, E = g.number_of_nodes(), g.number_of_edges()
    gen = torch.Generator(device=DEV).manual_seed(0)
    x = torch.randn(n, H, D, device=DEV, generator=gen)
    y = torch.randn(n, H, D, device=DEV, generator=gen)
    el, er = torch.randn(n, H, device=DEV, generator=gen), torch.randn(n, H, device=DEV, generator=gen)
    out = torch.empty(n, H, D, device=DEV)
    hbuf = torch.empty(n, 2 * H * D, dtype=torch.float16, device=DEV)
    dot = torch.empty(E, H, device=DEV)
    one = torch.ones(1, device=DEV)
    assert _C.spmm_dot_halves_fits(x, y, hbuf, D, H * D)
    lines = []
    try:
        for p in (0.0, 0.1):
            a = _C.gat_attn_fwd(g.csc, el, er, None, None, None, 0.2, H, None, drop=(p, 12345) if p > 0 else None)
            a = a[1] if p > 0 else a
            zeros = float((a == 0).float().mean())
            sweeps = {"spmm fwd": lambda: _C.spmm(g.csc, x, a, None, out=out),
                      "spmm_dot_halves bwd": lambda: _C.spmm_dot_halves(g.csr, x, a, g.csr2csc, y, one, hbuf, D, H * D, dot=dot)}
            for name, fn in sweeps.items():
                ms = {0: [], 1: []}
                for _ in range(REPEATS):
                    for on in (0, 1):
                        _C.spmm_set_zero_skip(on)
                        ms[on].append(median_ms(fn))
                kernel = _C._lib.bot_last_kernel().decode()
                med = {on: sorted(v)[len(v) // 2] for on, v in ms.items()}
                lines.append({"graph": "arxiv", "N": n, "E": E, "H": H, "D": D, "sweep": name, "kernel": kernel, "attn_drop": p,
                              "zero_weights": round(zeros, 4), "repeats": REPEATS, "iters": ITERS,
                              "off_ms": round(med[0], 4), "on_ms": round(med[1], 4), "gain": round(1 - med[1] / med[0], 4),
                              "off_min_max_ms": [round(min(ms[0]), 4), round(max(ms[0]), 4)],
                              "on_min_max_ms": [round(min(ms[1]), 4), round(max(ms[1]), 4)],
                              "gathered_TBs_off": round(E * H * D * 4 / med[0] / 1e9, 2)})
                print(json.dumps(lines[-1]), flush=True)
    finally:
        _C.spmm_set_zero_skip(1)
    with open(out_path, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
