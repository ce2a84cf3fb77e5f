"""Dot-product attention with edge features (bot_amd.ops.dot_attention_edge / nn.EdgeTransformerConv / nn.EdgeUniMP,
csrc/dot_attn.hip, the EDGE instances) measured on one GPU, with the protocol of tools/bench_dot_attn.py.

  op-arxiv-3x250 / op-arxiv-1x256 / op-proteins   `ops.dot_attention_edge` forward and forward + backward (q, k, v, weight), the kernel
            form against the tensor form, on the workload's graph with seeded K = 8 edge features (S-proteins at the largest of
            --proteins-scales at which the tensor form's [E, H, D] tensors fit, with H x D = 4 x 64).  The two forms alternate in ONE process:
            --rounds rounds, each the median of --calls calls after --warmup warm-up calls, every call ended by a device synchronise;
            the spread of a form is its largest minus its smallest round.  Peak allocated bytes of both forms beside the times, and
            `kernel_wins_beyond_tensor_spread`: the rule the default form follows.  Then the two edge sweeps (`_C.dot_attn_edge`,
            `_C.dot_attn_edge_bwd_dst`) beside the plain ones (`_C.dot_attn`, `_C.dot_attn_bwd_dst`) on the same graph and width: time,
            byte model (csrc/dot_attn.hip), the rate that model gives, and the ratio of the times next to the
            ratio of the byte models.
  sweeps-proteins  the four sweeps alone on S-proteins at --step-scale (4 x 64), where the tensor form does not fit.
  step-proteins  one full-batch train step of `workloads.build_unimp_edge("proteins")` beside `workloads.build_gen_edge("proteins")`'s,
            in the same process, at --step-scale.

Every step is a child process under its own `timeout -k 10`; the first one that fails or runs out of time ends the run (nothing more
is started on the GPU after a fault).

    python tools/bench_dot_attn_edge.py [--steps op-arxiv-3x250 op-arxiv-1x256 op-proteins sweeps-proteins step-proteins]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools.bench_dot_attn import DEV, _alternate, _graph, _operands, _peak  # noqa: E402

K = 8


def _edge_operands(g, H, a):
    gen = torch.Generator().manual_seed(a.seed + 6)
    n, E = g.number_of_nodes(), g.number_of_edges()
    ef = torch.rand(E, K, generator=gen).to(DEV)                                     # edge-id order
    qe, daef = ((0.5 * torch.randn(n, H * K, generator=gen)).to(DEV).view(n, H, K) for _ in range(2))
    return ef, qe, daef


def _sweeps(g, H, D, a):
    """The two edge sweeps and the two plain ones as callables over fixed operands, with their byte models."""
    from bot_amd import _C, ops
    n, E, HD, HK = g.number_of_nodes(), g.number_of_edges(), H * D, H * K
    q, k, v, dout = _operands(g, H, D, a)
    ef, qe, daef = _edge_operands(g, H, a)
    ef_pos = ops.edge_features_csc(g, ef)
    sc = D ** -0.5
    out, lse = _C.dot_attn(g.csc, q, k, v, sc)
    dq, pw, ds = _C.dot_attn_bwd_dst(g.csc, q, k, v, sc, None, 0.0, dout, out, lse)
    oute, lsee, aef = _C.dot_attn_edge(g.csc, q, k, v, qe, ef_pos, sc)
    dqx, dqe, pwe, dse = _C.dot_attn_edge_bwd_dst(g.csc, q, k, v, qe, ef_pos, sc, None, 0.0, dout, daef, oute, lsee, aef)
    forms = {"fwd": lambda: _C.dot_attn(g.csc, q, k, v, sc, out=out, lse=lse),
             "fwd_edge": lambda: _C.dot_attn_edge(g.csc, q, k, v, qe, ef_pos, sc, out=oute, lse=lsee, aef=aef),
             "bwd_dst": lambda: _C.dot_attn_bwd_dst(g.csc, q, k, v, sc, None, 0.0, dout, out, lse, dq=dq, pw=pw, ds=ds),
             "bwd_dst_edge": lambda: _C.dot_attn_edge_bwd_dst(g.csc, q, k, v, qe, ef_pos, sc, None, 0.0, dout, daef, oute, lsee, aef, dq=dqx, dqe=dqe,
                                                              pw=pwe, ds=dse)}
    model = {"fwd": 4 * (E * (1 + 2 * HD) + n * (2 * HD + H)), "fwd_edge": 4 * (E * (1 + 2 * HD + K) + n * (2 * HD + H + 2 * HK)),
             "bwd_dst": 4 * (E * (1 + 2 * HD + 2 * H) + n * (4 * HD + 2 * H)),
             "bwd_dst_edge": 4 * (E * (1 + 2 * HD + K + 2 * H) + n * (4 * HD + 2 * H + 4 * HK))}
    return forms, model, (q, k, v, dout, ef)


def child_op(name, H, D, scale, a, forms_too=True):
    from bot_amd import ops
    g = _graph(name, scale, a)
    n, E = g.number_of_nodes(), g.number_of_edges()
    forms, model, (q, k, v, dout, ef) = _sweeps(g, H, D, a)
    out = {"step": a.child, "graph": name, "scale": scale, "n_nodes": n, "n_edges": E, "H": H, "D": D, "K": K, "rounds": a.rounds,
           "calls": a.calls, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    gen = torch.Generator().manual_seed(a.seed + 7)
    W = ((K ** -0.5) * torch.randn(H * D, K, generator=gen)).to(DEV)
    leaves = [t.clone().requires_grad_() for t in (q, k, v, W)]

    def fwd(impl):
        with torch.no_grad():
            return ops.dot_attention_edge(g, q, k, v, ef, W, impl=impl)

    def both(impl):
        for t in leaves:
            t.grad = None
        ops.dot_attention_edge(g, leaves[0], leaves[1], leaves[2], ef, leaves[3], impl=impl).backward(dout)
    if forms_too:
        both("tensor")                    # does the tensor form run here at all?  (before anything is timed)
        torch.cuda.synchronize()
    sweeps = _alternate(forms, a)
    for key, val in sweeps.items():
        val["byte_model"] = model[key]
        val["model_gb_per_s"] = round(model[key] / (val["median_ms"] * 1e-3) / 1e9, 1)
    out["sweeps"] = sweeps
    for key in ("fwd", "bwd_dst"):
        out[f"{key}_edge_over_plain"] = {"time": round(sweeps[key + "_edge"]["median_ms"] / sweeps[key]["median_ms"], 4),
                                         "byte_model": round(model[key + "_edge"] / model[key], 4)}
    del forms
    if not forms_too:
        return out
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


def child_proteins(a):
    """The op on S-proteins at the largest of --proteins-scales at which the tensor form fits (an out-of-memory error, or the tensor form's
    refusal to differentiate a gather of more than 2^24 positions, moves on to the next; the scales that did not fit are recorded)."""
    too_large = []
    for scale in a.proteins_scales:
        try:
            out = child_op("proteins", 4, 64, scale, a)
            out["tensor_form_did_not_fit_at"] = too_large
            return out
        except (torch.OutOfMemoryError, ValueError) as e:
            # out of memory, or more than 2^24 positions: graph.take_rows gathers those in pieces, which carry no gradient
            if not isinstance(e, torch.OutOfMemoryError) and "has no gradient on a graph" not in str(e):
                raise
            too_large.append({"scale": scale, "why": type(e).__name__ + ": " + str(e)[:120]})
            torch.cuda.empty_cache()
    sys.exit(f"the tensor form fits at none of {a.proteins_scales}")


def child_step(a):
    from bot_amd import workloads
    out = {"step": "step-proteins", "scale": a.step_scale, "rounds": a.rounds, "calls": a.calls, "warmup": a.warmup}
    for key, make in (("unimp_edge", lambda: workloads.build_unimp_edge("proteins", DEV, scale=a.step_scale, seed=a.seed)),
                      ("gen_edge", lambda: workloads.build_gen_edge("proteins", DEV, scale=a.step_scale, seed=a.seed))):
        wl = make()
        out["n_nodes"], out["n_edges"] = wl.n_nodes, wl.n_edges
        out[key] = dict(_alternate({"step": wl.step}, a)["step"], describe=wl.describe, peak_bytes=_peak(wl.step))
        del wl
        torch.cuda.empty_cache()
    return out


CHILDREN = {
    "op-arxiv-3x250": lambda a: child_op("arxiv", 3, 250, a.scale, a),
    "op-arxiv-1x256": lambda a: child_op("arxiv", 1, 256, a.scale, a),
    "op-proteins": child_proteins,
    "sweeps-proteins": lambda a: child_op("proteins", 4, 64, a.step_scale, a, forms_too=False),
    "step-proteins": child_step,
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", nargs="+", default=list(CHILDREN), choices=list(CHILDREN))
    ap.add_argument("--scale", type=float, default=1.0, help="of S-arxiv")
    ap.add_argument("--proteins-scales", type=float, nargs="+", default=[0.5, 0.25, 0.125, 0.0625],
                    help="of S-proteins, largest first: the op runs at the first at which the tensor form fits")
    ap.add_argument("--step-scale", type=float, default=1.0, help="of S-proteins for the train steps")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=420, help="seconds a step's child process may run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_dot_attn_edge.jsonl"))
    ap.add_argument("--child", metavar="STEP", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        if not torch.cuda.is_available():
            sys.exit("bench_dot_attn_edge.py measures on an MI355X: no GPU here")
        print("RESULT " + json.dumps(CHILDREN[a.child](a)), flush=True)
        return
    passed = [x for x in sys.argv[1:]]
    with open(a.out, "a") as f:
        for step in a.steps:
            cmd = [sys.executable, os.path.abspath(__file__)] + passed + ["--child", step]
            out = subprocess.run(["timeout", "-k", "10", str(a.timeout)] + cmd, cwd=ROOT, capture_output=True, text=True)
            lines = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
            if out.returncode != 0 or not lines:
                sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
                sys.exit(f"{step}: child ended with rc {out.returncode}; stopping here")
            result = json.loads(lines[-1][7:])
            print(json.dumps(result), flush=True)
            f.write(json.dumps(result) + "\n")
            f.flush()


if __name__ == "__main__":
    main()
