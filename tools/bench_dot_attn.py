"""Dot-product attention (bot_amd.ops.dot_attention / nn.TransformerConv / nn.DotGatConv / nn.UniMP, csrc/dot_attn.hip) measured on one GPU.

  op-arxiv-3x250 / op-arxiv-1x256 / op-products   `ops.dot_attention` forward and forward + backward (all three gradients), the kernel
            form against the tensor form (`(k[src] * q[dst]).sum(-1) * scale` -> `gat_attention(ee=)` -> `u_mul_e_sum`), on the
            workload's graph (S-products at --products-scale, with H x D = 4 x 120).  The two forms alternate in ONE process: --rounds
            rounds, each the median of --calls calls after --warmup warm-up calls, every call ended by a device synchronise; the spread
            of a form is its largest minus its smallest round.  Peak allocated bytes of both forms beside the times, and
            `kernel_wins_beyond_tensor_spread`: the rule `ops.dot_attn_default_impl` is set by.  Then the three sweeps alone
            (`_C.dot_attn`, `_C.dot_attn_bwd_dst`, `_C.dot_attn_bwd_src`) and the shared (k is v) forward beside the sum sweep
            (`_C.spmm` on g.csc / g.csr) at the same width, each with its byte model (csrc/dot_attn.hip) and the rate that model gives.
  step-arxiv     one full-batch train step of `workloads.build_unimp("arxiv")` beside `workloads.build("arxiv")`'s and
            `workloads.build_gatv2("arxiv")`'s own steps, in the same process.
  sampled-arxiv  one sampled batch (sample + step) of `build_unimp("arxiv", sampled=True)` beside `build_sampled("arxiv")`.
  trace     one `rocprofv3 --kernel-trace --stats` run of a child that calls the sweeps and the sum sweep once on S-arxiv at 3 x 250
            (no counters in that run); their rows of the kernel statistics go to bench_dot_attn_kernel_stats.csv beside --out.

Every step is a child process under its own `timeout -k 10`; the first one that fails or runs out of time ends the run (nothing more
is started on the GPU after a fault).

    python tools/bench_dot_attn.py [--steps op-arxiv-3x250 op-arxiv-1x256 op-products step-arxiv sampled-arxiv trace]
"""
import argparse
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

DEV = "cuda:0"


def _sync():
    torch.cuda.synchronize()
    return time.perf_counter()


def _median_ms(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(calls):
        t0 = _sync()
        fn()
        times.append(_sync() - t0)
    return 1e3 * statistics.median(times)


def _alternate(forms, a):
    """{name: {"rounds_ms", "median_ms", "spread_ms"}} of forms {name: callable}, alternating round by round."""
    rounds = {k: [] for k in forms}
    for _ in range(a.rounds):
        for k, fn in forms.items():
            rounds[k].append(round(_median_ms(fn, a.calls, a.warmup), 4))
    return {k: {"rounds_ms": v, "median_ms": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4)} for k, v in rounds.items()}


def _graph(name, scale, a):
    """The workload's graph (the same seeded edges and preprocessing as bot_amd.workloads) without its feature matrix."""
    import bot_amd
    from bot_amd import synth
    n, e_raw, _, _ = synth.SHAPES[name]
    n, e_raw = max(8, int(n * scale)), max(8, int(e_raw * scale))
    s, d = synth.powerlaw_edges(n, e_raw, synth.BASE_SEED + a.seed, device=DEV)
    g = bot_amd.preprocess(bot_amd.Graph(s, d, n))
    _ = g.csr2csc
    return g


def _operands(g, H, D, a):
    gen = torch.Generator().manual_seed(a.seed + 5)
    n = g.number_of_nodes()
    return tuple((0.5 * torch.randn(n, H * D, generator=gen)).to(DEV).view(n, H, D) for _ in range(4))       # q, k, v, dout


def _sweeps(g, H, D, a):
    """The three sweeps, the shared forward and the sum sweep in both directions as callables over fixed operands, with their byte
    models."""
    from bot_amd import _C
    n, E, HD = g.number_of_nodes(), g.number_of_edges(), H * D
    q, k, v, dout = _operands(g, H, D, a)
    sc = D ** -0.5
    out, lse = _C.dot_attn(g.csc, q, k, v, sc)
    dq, pw, ds = _C.dot_attn_bwd_dst(g.csc, q, k, v, sc, None, 0.0, dout, out, lse)
    dk, dv = torch.empty_like(k), torch.empty_like(v)
    out2, lse2 = torch.empty_like(out), torch.empty_like(lse)
    forms = {"fwd": lambda: _C.dot_attn(g.csc, q, k, v, sc, out=out, lse=lse),
             "fwd_shared": lambda: _C.dot_attn(g.csc, q, k, k, sc, out=out2, lse=lse2),
             "bwd_dst": lambda: _C.dot_attn_bwd_dst(g.csc, q, k, v, sc, None, 0.0, dout, out, lse, dq=dq, pw=pw, ds=ds),
             "bwd_src": lambda: _C.dot_attn_bwd_src(g.csr, g.csr2csc, q, dout, pw, ds, sc, dk=dk, dv=dv),
             "sum_csc": lambda: _C.spmm(g.csc, k), "sum_csr": lambda: _C.spmm(g.csr, q)}
    model = {"fwd": 4 * (E * (1 + 2 * HD) + n * (2 * HD + H)), "fwd_shared": 4 * (E * (1 + HD) + n * (2 * HD + H)),
             "bwd_dst": 4 * (E * (1 + 2 * HD + 2 * H) + n * (4 * HD + 2 * H)), "bwd_src": 4 * (E * (2 + 2 * HD + 2 * H) + 3 * n * HD),
             "sum_csc": 4 * (E * (1 + HD) + n * HD), "sum_csr": 4 * (E * (1 + HD) + n * HD)}
    return forms, model, (q, k, v, dout)


def _peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def child_op(name, H, D, scale, a):
    from bot_amd import ops
    g = _graph(name, scale, a)
    n, E = g.number_of_nodes(), g.number_of_edges()
    forms, model, (q, k, v, dout) = _sweeps(g, H, D, a)
    out = {"step": a.child, "graph": name, "scale": scale, "n_nodes": n, "n_edges": E, "H": H, "D": D, "rounds": a.rounds, "calls": a.calls,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    sweeps = _alternate(forms, a)
    for key, val in sweeps.items():
        val["byte_model"] = model[key]
        val["model_gb_per_s"] = round(model[key] / (val["median_ms"] * 1e-3) / 1e9, 1)
    out["sweeps"] = sweeps
    for key, ref in (("fwd", "sum_csc"), ("fwd_shared", "sum_csc"), ("bwd_dst", "sum_csc"), ("bwd_src", "sum_csr")):
        out[f"{key}_rate_over_sum_sweep"] = round(sweeps[key]["model_gb_per_s"] / sweeps[ref]["model_gb_per_s"], 4)
    out["shared_forward_over_unshared"] = round(sweeps["fwd_shared"]["median_ms"] / sweeps["fwd"]["median_ms"], 4)
    del forms
    leaves = [t.clone().requires_grad_() for t in (q, k, v)]

    def fwd(impl):
        with torch.no_grad():
            return ops.dot_attention(g, q, k, v, impl=impl)

    def both(impl):
        for t in leaves:
            t.grad = None
        ops.dot_attention(g, *leaves, impl=impl).backward(dout)
    impls = ("kernel", "tensor")
    diff = float((fwd("kernel") - fwd("tensor")).abs().max())
    if not diff <= 1e-3:
        sys.exit(f"the two forms differ by {diff}")
    out["max_abs_diff_between_forms"] = diff
    out["forward"] = _alternate({key: (lambda key=key: fwd(key)) for key in impls}, a)
    out["forward_backward"] = _alternate({key: (lambda key=key: both(key)) for key in impls}, a)
    out["peak_bytes_forward_backward"] = {key: _peak(lambda key=key: both(key)) for key in impls}
    wins = True
    for key in ("forward", "forward_backward"):
        r = out[key]
        r["kernel_faster_by_ms"] = round(r["tensor"]["median_ms"] - r["kernel"]["median_ms"], 4)
        wins = wins and r["kernel_faster_by_ms"] > r["tensor"]["spread_ms"]
    out["kernel_wins_beyond_tensor_spread"] = wins
    return out


def child_step(a):
    from bot_amd import workloads
    out = {"step": "step-arxiv", "rounds": a.rounds, "calls": a.calls, "warmup": a.warmup}
    for key, make in (("unimp", lambda: workloads.build_unimp("arxiv", DEV, scale=a.scale, seed=a.seed)),
                      ("build", lambda: workloads.build("arxiv", DEV, scale=a.scale, seed=a.seed)),
                      ("gatv2", lambda: workloads.build_gatv2("arxiv", DEV, scale=a.scale, seed=a.seed))):
        wl = make()
        out["n_nodes"], out["n_edges"] = wl.n_nodes, wl.n_edges
        out[key] = dict(_alternate({"step": wl.step}, a)["step"], describe=wl.describe, peak_bytes=_peak(wl.step))
        del wl
        torch.cuda.empty_cache()
    return out


def child_sampled(a):
    from bot_amd import workloads
    out = {"step": "sampled-arxiv", "rounds": a.rounds, "calls": a.calls, "warmup": a.warmup}
    for key, make in (("unimp", lambda: workloads.build_unimp("arxiv", DEV, sampled=True, scale=a.scale, seed=a.seed)),
                      ("build_sampled", lambda: workloads.build_sampled("arxiv", DEV, scale=a.scale, seed=a.seed))):
        wl = make()
        it = [iter(wl.loader)]

        def batch():
            try:
                _, output_nodes, blocks = next(it[0])
            except StopIteration:
                it[0] = iter(wl.loader)
                _, output_nodes, blocks = next(it[0])
            wl.step(blocks, output_nodes)
        out[key] = dict(_alternate({"batch": batch}, a)["batch"], describe=wl.describe)
        del wl
        torch.cuda.empty_cache()
    return out


def child_trace(a):
    g = _graph("arxiv", a.scale, a)
    forms, model, _ = _sweeps(g, 3, 250, a)
    for fn in forms.values():
        fn()
    torch.cuda.synchronize()
    return {"step": "trace", "n_nodes": g.number_of_nodes(), "n_edges": g.number_of_edges(), "H": 3, "D": 250, "calls": 1}


CHILDREN = {
    "op-arxiv-3x250": lambda a: child_op("arxiv", 3, 250, a.scale, a),
    "op-arxiv-1x256": lambda a: child_op("arxiv", 1, 256, a.scale, a),
    "op-products": lambda a: child_op("products", 4, 120, a.products_scale, a),
    "step-arxiv": child_step, "sampled-arxiv": child_sampled, "trace": child_trace,
}


def _kernel_stats(directory, out_csv):
    """The sweeps' rows of the run's kernel statistics -> out_csv; returns {kernel: calls and average ns}."""
    import csv
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        return {}
    rows = list(csv.DictReader(open(files[0])))
    keep = [r for r in rows if "dot_attn" in r.get("Name", "") or "spmm" in r.get("Name", "")]
    if keep:
        with open(out_csv, "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=list(keep[0]))
            w.writeheader()
            w.writerows(keep)
    return {r["Name"].split("(")[0].split("::")[-1]: {"calls": int(r["Calls"]), "average_ns": float(r["AverageNs"])} for r in keep}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", nargs="+", default=["op-arxiv-3x250", "op-arxiv-1x256", "op-products", "step-arxiv", "sampled-arxiv", "trace"], choices=list(CHILDREN))
    ap.add_argument("--scale", type=float, default=1.0, help="of S-arxiv")
    ap.add_argument("--products-scale", type=float, default=0.1, help="of S-products where the tensor form runs too")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=420, help="seconds a step's child process may run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_dot_attn.jsonl"))
    ap.add_argument("--child", metavar="STEP", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        if not torch.cuda.is_available():
            sys.exit("bench_dot_attn.py measures on an MI355X: no GPU here")
        print("RESULT " + json.dumps(CHILDREN[a.child](a)), flush=True)
        return
    passed = [x for x in sys.argv[1:]]
    with open(a.out, "a") as f:
        for step in a.steps:
            cmd = [sys.executable, os.path.abspath(__file__)] + passed + ["--child", step]
            tmp = None
            if step == "trace":
                tmp = tempfile.mkdtemp(prefix="bench_dot_attn_trace_")
                cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--"] + cmd
            out = subprocess.run(["timeout", "-k", "10", str(a.timeout)] + cmd, cwd=ROOT, capture_output=True, text=True)
            lines = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
            if out.returncode != 0 or not lines:
                sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
                sys.exit(f"{step}: child ended with rc {out.returncode}; stopping here")
            result = json.loads(lines[-1][7:])
            if tmp is not None:
                result["kernels"] = _kernel_stats(tmp, os.path.join(os.path.dirname(a.out), "bench_dot_attn_kernel_stats.csv"))
            print(json.dumps(result), flush=True)
            f.write(json.dumps(result) + "\n")
            f.flush()


if __name__ == "__main__":
    main()
