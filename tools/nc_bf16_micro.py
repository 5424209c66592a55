#!/usr/bin/env python3
"""The MMA layer with fp32 and with bf16 logit tables (MMA(..., logit_dtype=)) on bench.py's C4-shape synthetic graph (R-MAT scale 20,
5 M undirected edges, H = 128, sum / mean / max / min, hash dropout 0.5).  THREE forms in ONE process, interleaved rounds after a warm-up:
fp32 tables; bf16 tables through the conversion pass (dense.BF16_EPILOGUE = False: fp32 forward GEMM + mma_rows_to_bf16); bf16 tables
written by the forward GEMM's epilogue (the default).
  * the layer's forward + backward step of each form, HIP events around `--steps` steps per round (bench.py's default step count or more);
  * the forward GEMM [P|Q] = x [Wtop|Wbot] alone, fp32-out and bf16-out (dense.mm_into), events around `--reps` back-to-back calls;
  * the conversion launch (mma_rows_to_bf16 of the (N, 2*K*H) fp32 output) the conversion form pays;
  * the two fused calls on their own (K1: mma_nc_fused_fwd[_h]; K2b with the node-level epilogue: mma_nc_fused_bwd[_h]) on prepared tables.
Prints one JSON line: median and [min, max] ms of each, the ratios and the device name.

    python tools/nc_bf16_micro.py [--rounds 5] [--steps 10] [--reps 10] [--scale 20 --edges 5000000 --hidden 128]   (on the GPU box)"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mma_amd  # noqa: E402
from bench import C4_DEFAULTS, make_layer  # noqa: E402
from mma_amd import dense  # noqa: E402
from mma_amd import functional as Fn  # noqa: E402
from tools.synth import feature_rows, rmat_graph  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--scale", type=int, default=C4_DEFAULTS["scale"])
ap.add_argument("--edges", type=int, default=C4_DEFAULTS["edges"])
ap.add_argument("--hidden", type=int, default=C4_DEFAULTS["hidden"])
ap.add_argument("--aggregators", default=C4_DEFAULTS["aggregators"])
ap.add_argument("--dropout", type=float, default=C4_DEFAULTS["dropout"])
args = ap.parse_args()

dev = torch.device("cuda:0")
names = args.aggregators.split(",")
K, H, C = len(names), args.hidden, C4_DEFAULTS["nclass"]
KH = K * H
rowptr, col = rmat_graph(args.scale, args.edges, seed=42)
N, E = len(rowptr) - 1, int(rowptr[-1])
rp_d, cl_d = torch.from_numpy(np.ascontiguousarray(rowptr)).to(dev), torch.from_numpy(np.ascontiguousarray(col)).to(dev)
graph = mma_amd.NCGraph.from_device_csr(rp_d, cl_d, H=H)
adj = mma_amd.graph.SpmmGraph.from_device_csr(rp_d, cl_d)
x = torch.from_numpy(feature_rows(0, N, H, 42)).to(dev).requires_grad_(True)
cot = torch.from_numpy(feature_rows(0, N, C, 43, relu=False)).to(dev)

torch.manual_seed(42)
layers = {"fp32": make_layer(mma_amd, graph, H, C, names, args.dropout, dev),
          "bf16": make_layer(mma_amd, graph, H, C, names, args.dropout, dev, logit_dtype=torch.bfloat16)}
with torch.no_grad():
    for a, b in zip(layers["fp32"].owned, layers["bf16"].owned):
        b.copy_(a)


def timed(fn, n):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(n):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / n


def layer_step(layer, epilogue=True):
    def step():
        dense.BF16_EPILOGUE = epilogue
        x.grad = None
        for prm in layer.owned:
            prm.grad = None
        layer(x, adj).backward(cot)
    return step


# the two fused calls on prepared tables (bench.py::fused_calls_in_graph's operands)
kinds, acts = layers["fp32"]._codes(names)
with torch.no_grad():
    PQ32 = x.detach() @ Fn.mask_weights([getattr(layers["fp32"], "mask_" + n).detach() for n in names])
tables = {"fp32": PQ32, "bf16": Fn.rows_to_bf16(PQ32)}
drop = Fn.DropoutSpec(args.dropout, seed=1234)
g = torch.randn(N, H, device=dev)
gPQ = torch.empty((N, 2 * KH), device=dev)
gx = torch.empty((N, H), device=dev)
partial = torch.empty((graph.t_n_slots, (K + 1) * H), device=dev) if graph.t_n_slots else None
state = {}


def fwd(tag):
    PQ = tables[tag]
    return lambda: state.__setitem__(tag, Fn.nc_fwd_launch(x.detach(), PQ[:, :KH], PQ[:, KH:], graph, kinds, acts, drop, True, True))


def bwd(tag):
    PQ = tables[tag]

    def run():
        _, T, _, crow = state[tag]
        Fn.nc_bwd_edges_launch(x.detach(), PQ[:, :KH], PQ[:, KH:], None, g, crow, None, graph, kinds, acts, drop, gPQ[:, KH:], gx, partial,
                               T=T, gP=gPQ[:, :KH])
    return run


# the forward GEMM alone: the same operands into an fp32 and into a bf16 [P|Q] (the epilogue form)
wcat = Fn.mask_weights([getattr(layers["fp32"], "mask_" + n).detach() for n in names])
gemm_out = {"fp32": torch.empty((N, 2 * KH), device=dev), "bf16": torch.empty((N, 2 * KH), device=dev, dtype=torch.bfloat16)}
gemm_form = dense.nn_form(N, H, 2 * KH)


def gemm(tag):
    def run():
        dense.BF16_EPILOGUE = True
        dense.mm_into(x.detach(), wcat, gemm_out[tag])
    return run


work = {"step_fp32": (layer_step(layers["fp32"]), args.steps),
        "step_bf16_conversion": (layer_step(layers["bf16"], epilogue=False), args.steps),
        "step_bf16_epilogue": (layer_step(layers["bf16"], epilogue=True), args.steps)}
for tag in ("fp32", "bf16"):
    work["gemm_fwd_" + tag + "_out"] = (gemm(tag), args.reps)
    work["nc_fused_fwd_" + tag] = (fwd(tag), args.reps)
    work["nc_fused_bwd_" + tag] = (bwd(tag), args.reps)
work["rows_to_bf16"] = (lambda: Fn.rows_to_bf16(PQ32, tables["bf16"]), args.reps)

for name, (fn, n) in work.items():           # warm-up: plans, allocator, code objects; the forward before its backward
    for _ in range(args.warmup):
        fn()
torch.cuda.synchronize()
ms = {name: [] for name in work}
for _ in range(args.rounds):                  # interleaved: a drifting clock or a busy neighbour hits both sides alike
    for name, (fn, n) in work.items():
        ms[name].append(timed(fn, n))
med = {name: statistics.median(v) for name, v in ms.items()}
out = {"device": torch.cuda.get_device_name(0), "N": N, "E": E, "H": H, "K": K, "dropout": args.dropout, "rounds": args.rounds,
       "steps": args.steps, "reps": args.reps, "median_ms": {k: round(v, 4) for k, v in med.items()},
       "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
       "forward_gemm_form": gemm_form,
       "bf16_over_fp32": dict({k: round(med[k + "_bf16"] / med[k + "_fp32"], 4) for k in ("nc_fused_fwd", "nc_fused_bwd")},
                              gemm_fwd=round(med["gemm_fwd_bf16_out"] / med["gemm_fwd_fp32_out"], 4),
                              step_conversion=round(med["step_bf16_conversion"] / med["step_fp32"], 4),
                              step_epilogue=round(med["step_bf16_epilogue"] / med["step_fp32"], 4)),
       "epilogue_over_conversion_step": round(med["step_bf16_epilogue"] / med["step_bf16_conversion"], 4)}
dense.BF16_EPILOGUE = True
print(json.dumps(out))
