"""R-GCN (bot_amd.ops.rel_expand_sum / rel_contract_sum, nn.RelGraphConv / nn.RGCN, csrc/spmm_rel.hip) measured on one GPU.

  op-arxiv / op-reddit   each sweep, forward and forward + backward (the gradients of the features and, with a basis, of coef), at F = 256
            with a basis (R, B) = (8, 4) and one-hot R = 8, in three forms: the kernel form, the tensor form (torch ops over [E, F]
            messages) and the LOOP form - what the tree offered before these kernels: B calls of `ops.u_mul_e_sum` with the weight column
            c_e coef[r_e, b].  The forms alternate in ONE process: --rounds rounds, each the median of --calls calls after --warmup warm-up
            calls, every call ended by a device synchronise; the spread of a form is its largest minus its smallest round.
            `kernel_wins_beyond_loop_spread` is the rule `ops.rel_default_impl` is set by.  On S-reddit the tensor form is left out (its
            [E, F] tensors are 117 GB each, and beyond 2^24 edges its gathers carry no gradient).  Then the two sweeps alone (`_C.spmm_rel_*`)
            beside the sum sweep (`_C.spmm`) at the same gathered width, each with its byte model (csrc/spmm_rel.hip) and the rate it gives.
  step-arxiv     one full-batch train step of `workloads.build_rgcn("arxiv")`, basis and one-hot.
  trace-arxiv    five such steps and nothing else: the child to run under `rocprofv3 --kernel-trace --stats` for the sweeps' share.

Every step is a child process under its own `timeout -k 10`; the first one that fails or runs out of time ends the run (nothing more
is started on the GPU after a fault).

    python tools/bench_rgcn.py [--steps op-arxiv op-reddit step-arxiv]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

DEV = "cuda:0"
R, B = 8, 4


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
    _ = g.csr
    return g


def child_op(name, F, scale, a, with_tensor):
    from bot_amd import _C, ops
    from bot_amd import nn as bnn
    g = _graph(name, scale, a)
    n, E = g.number_of_nodes(), g.number_of_edges()
    gen = torch.Generator().manual_seed(a.seed + 5)
    et = torch.randint(0, R, (E,), generator=gen, dtype=torch.int32).to(DEV)
    nm = bnn.rel_norm(g, et, R).view(-1)
    x = torch.randn(n, F, generator=gen).to(DEV)
    y = torch.randn(n, R, F, generator=gen).to(DEV)                  # basis mode reads its first B blocks
    coef0 = torch.randn(R, B, generator=gen).to(DEV)
    out = {"step": a.child, "graph": name, "scale": scale, "n_nodes": n, "n_edges": E, "F": F, "R": R, "B": B, "rounds": a.rounds,
           "calls": a.calls, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    # ---- the sweeps alone beside the sum sweep at the gathered width
    et_c, nm_c = ops._rel_positions(g, et, "csc"), ops._rel_positions(g, nm, "csc")
    yb = y[:, :B].contiguous()
    forms = {"expand_basis": lambda: _C.spmm_rel_expand(g.csc, x, et_c, R, coef0, nm_c),
             "expand_onehot": lambda: _C.spmm_rel_expand(g.csc, x, et_c, R, None, nm_c),
             "contract_basis": lambda: _C.spmm_rel_contract(g.csc, yb, et_c, R, coef0, nm_c),
             "contract_onehot": lambda: _C.spmm_rel_contract(g.csc, y, et_c, R, None, nm_c),
             "sum_F": lambda: _C.spmm(g.csc, x.view(n, 1, F)), "sum_BF": lambda: _C.spmm(g.csc, yb.view(n, 1, B * F))}
    model = {"expand_basis": 4 * (E * (3 + F) + n * B * F), "expand_onehot": 4 * (E * (3 + F) + n * R * F),
             "contract_basis": 4 * (E * (3 + B * F) + n * F), "contract_onehot": 4 * (E * (3 + F) + n * F),
             "sum_F": 4 * (E * (1 + F) + n * F), "sum_BF": 4 * (E * (1 + B * F) + n * B * F)}
    sweeps = _alternate(forms, a)
    for key, val in sweeps.items():
        val["byte_model"] = model[key]
        val["model_gb_per_s"] = round(model[key] / (val["median_ms"] * 1e-3) / 1e9, 1)
    out["sweeps"] = sweeps
    for key, ref in (("expand_basis", "sum_F"), ("expand_onehot", "sum_F"), ("contract_basis", "sum_BF"), ("contract_onehot", "sum_F")):
        out[f"{key}_rate_over_sum_sweep"] = round(sweeps[key]["model_gb_per_s"] / sweeps[ref]["model_gb_per_s"], 4)
    del forms
    # ---- the three forms of each op
    impls = ("kernel", "tensor", "loop") if with_tensor else ("kernel", "loop")
    wins = True
    for mode in ("basis", "onehot"):
        coef = coef0.clone().requires_grad_() if mode == "basis" else None
        Bc = B if mode == "basis" else R
        leaves = {"expand": x.clone().requires_grad_(), "contract": y[:, :Bc].contiguous().requires_grad_()}
        ups = {"expand": torch.randn(n, Bc, F, generator=gen).to(DEV), "contract": torch.randn(n, F, generator=gen).to(DEV)}

        def weights():
            w = torch.nn.functional.one_hot(et.long(), R).to(torch.float32) if coef is None else coef[et.long()]
            return w * nm.unsqueeze(1)                               # [E, Bc], edge-id order

        def run(sweep, impl, t):
            if impl != "loop":
                return (ops.rel_expand_sum if sweep == "expand" else ops.rel_contract_sum)(g, t, et, R, coef, nm, impl=impl)
            w = weights()
            if sweep == "expand":
                return torch.stack([ops.u_mul_e_sum(g, t.view(n, 1, F), w[:, b].reshape(E, 1, 1)).view(n, F) for b in range(Bc)], dim=1)
            return sum(ops.u_mul_e_sum(g, t[:, b].reshape(n, 1, F), w[:, b].reshape(E, 1, 1)).view(n, F) for b in range(Bc))
        for sweep in ("expand", "contract"):
            t, up = leaves[sweep], ups[sweep]

            def fwd(impl):
                with torch.no_grad():
                    return run(sweep, impl, t)

            def both(impl):
                t.grad = None
                if coef is not None:
                    coef.grad = None
                run(sweep, impl, t).backward(up)
            ref = fwd("kernel")
            for impl in impls[1:]:
                diff = float((ref - fwd(impl)).abs().max())
                if not diff <= 1e-2:
                    sys.exit(f"{mode} {sweep}: the {impl} form differs from the kernel form by {diff}")
            del ref
            r = {"forward": _alternate({i: (lambda i=i: fwd(i)) for i in impls}, a),
                 "forward_backward": _alternate({i: (lambda i=i: both(i)) for i in impls}, a)}
            for key in ("forward", "forward_backward"):
                v = r[key]
                v["kernel_faster_than_loop_by_ms"] = round(v["loop"]["median_ms"] - v["kernel"]["median_ms"], 4)
                wins = wins and v["kernel_faster_than_loop_by_ms"] > v["loop"]["spread_ms"]
            out[f"{mode}_{sweep}"] = r
    out["kernel_wins_beyond_loop_spread"] = wins
    return out


def _workloads(a):
    from bot_amd import workloads
    return {"basis": workloads.build_rgcn("arxiv", DEV, scale=a.scale, seed=a.seed),
            "onehot": workloads.build_rgcn("arxiv", DEV, scale=a.scale, seed=a.seed, regularizer=None)}


def child_step(a):
    wls = _workloads(a)
    wl = wls["basis"]
    out = {"step": "step-arxiv", "rounds": a.rounds, "calls": a.calls, "warmup": a.warmup, "n_nodes": wl.n_nodes, "n_edges": wl.n_edges,
           "describe": wl.describe}
    out["forms"] = _alternate({k: (lambda w=w: w.step()) for k, w in wls.items()}, a)
    return out


def child_trace(a):
    wl = _workloads(a)["basis"]
    for _ in range(3):
        wl.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        wl.step()
    torch.cuda.synchronize()
    return {"step": "trace-arxiv", "steps": 5, "warmup_steps": 3, "ms_per_step": round(200 * (time.perf_counter() - t0), 3)}


CHILDREN = {
    "op-arxiv": lambda a: child_op("arxiv", 256, a.scale, a, True),
    "op-reddit": lambda a: child_op("reddit", 256, a.reddit_scale, a, False),
    "step-arxiv": child_step,
    "trace-arxiv": child_trace,
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", nargs="+", default=["op-arxiv", "op-reddit", "step-arxiv"], choices=list(CHILDREN))
    ap.add_argument("--scale", type=float, default=1.0, help="of S-arxiv")
    ap.add_argument("--reddit-scale", type=float, default=1.0, help="of S-reddit")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=420, help="seconds a step's child process may run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_rgcn.jsonl"))
    ap.add_argument("--child", metavar="STEP", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        if not torch.cuda.is_available():
            sys.exit("bench_rgcn.py measures on an MI355X: no GPU here")
        print("RESULT " + json.dumps(CHILDREN[a.child](a)), flush=True)
        return
    passed = [x for x in sys.argv[1:]]
    with open(a.out, "a") as f:
        for step in a.steps:
            cmd = [sys.executable, os.path.abspath(__file__)] + passed + ["--child", step]
            out = subprocess.run(["timeout", "-k", "10", str(a.timeout)] + cmd, cwd=ROOT, capture_output=True, text=True)
            lines = [line for line in out.stdout.splitlines() if line.startswith("RESULT ")]
            if out.returncode != 0 or not lines:
                sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
                sys.exit(f"{step}: child ended with rc {out.returncode}; stopping here")
            result = json.loads(lines[-1][7:])
            print(json.dumps(result), flush=True)
            f.write(json.dumps(result) + "\n")
            f.flush()


if __name__ == "__main__":
    main()
