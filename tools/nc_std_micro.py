#!/usr/bin/env python3
"""The `std` aggregator with fp32 and with bf16 logit tables on bench.py's C4-shape synthetic graph (R-MAT scale 20, 5 M undirected edges,
H = 128, ONE `std` mask, hash dropout 0.5): the sibling of tools/nc_bf16_micro.py for the second-moment kernels (csrc/nc_moments.hip),
same protocol - both forms in ONE process, interleaved rounds after a warm-up, HIP events, median and [min, max].
  * the two std calls on their own on prepared tables: K1s (mma_nc_std_fwd[_h], saving for the backward) and K2s (mma_nc_std_bwd[_h]:
    node pass + edge pass), events around `--reps` back-to-back calls;
  * the std node alone, forward + backward from (x, mask_std): today's fp32 path (two mm + nc_std_aggregate, as MMA._std runs it) against
    the one-node form with bf16 tables (Fn.nc_std_local) - and the one-node form with fp32 tables, to tell the node's share from the
    table type's;
  * the layer's forward + backward step with aggregator list ["std"] (MMA(..., strict_reference=False, logit_dtype=)), events around
    `--steps` steps per round.
Prints one JSON line: median and [min, max] ms of each, the ratios and the device name.

    python tools/nc_std_micro.py [--rounds 5] [--steps 10] [--reps 10] [--scale 20 --edges 5000000 --hidden 128]   (on the GPU box)"""
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
from mma_amd import functional as Fn  # noqa: E402
from mma_amd.dense import mm  # noqa: E402
from tools.synth import feature_rows, rmat_graph  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--scale", type=int, default=C4_DEFAULTS["scale"])
ap.add_argument("--edges", type=int, default=C4_DEFAULTS["edges"])
ap.add_argument("--hidden", type=int, default=C4_DEFAULTS["hidden"])
ap.add_argument("--dropout", type=float, default=C4_DEFAULTS["dropout"])
ap.add_argument("--activation", default="sigmoid", choices=["sigmoid", "new_sigmoid"], help="new_sigmoid: std takes the raw logits")
args = ap.parse_args()

dev = torch.device("cuda:0")
H, C = args.hidden, C4_DEFAULTS["nclass"]
rowptr, col = rmat_graph(args.scale, args.edges, seed=42)
N, E = len(rowptr) - 1, int(rowptr[-1])
rp_d, cl_d = torch.from_numpy(np.ascontiguousarray(rowptr)).to(dev), torch.from_numpy(np.ascontiguousarray(col)).to(dev)
graph = mma_amd.NCGraph.from_device_csr(rp_d, cl_d, H=H)
adj = mma_amd.graph.SpmmGraph.from_device_csr(rp_d, cl_d)
x = torch.from_numpy(feature_rows(0, N, H, 42)).to(dev).requires_grad_(True)
cot = torch.from_numpy(feature_rows(0, N, C, 43, relu=False)).to(dev)
g = torch.randn(N, H, device=dev)

torch.manual_seed(42)
layers = {"fp32": make_layer(mma_amd, graph, H, C, ["std"], args.dropout, dev, strict_reference=False),
          "bf16": make_layer(mma_amd, graph, H, C, ["std"], args.dropout, dev, strict_reference=False, logit_dtype=torch.bfloat16)}
with torch.no_grad():
    for a, b in zip(layers["fp32"].owned, layers["bf16"].owned):
        b.copy_(a)
for layer in layers.values():
    layer.activation = args.activation               # read at call time (bench.make_layer constructs with "new_sigmoid")
w = layers["fp32"].mask_std
act = Fn.ACT_RAW if args.activation == "new_sigmoid" else Fn.ACT_SIGMOID
drop = Fn.DropoutSpec(args.dropout, seed=1234)


def timed(fn, n):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(n):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / n


def layer_step(layer):
    def step():
        x.grad = None
        for prm in layer.owned:
            prm.grad = None
        layer(x, adj).backward(cot)
    return step


def node_step(form):
    """forward + backward of the std node alone from (x, mask_std), cotangent g."""
    def step():
        x.grad = None
        w.grad = None
        if form == "two_mm_fp32":
            m = Fn.nc_std_aggregate(x, mm(x, w[:H]), mm(x, w[H:]), graph, act, drop)
        else:
            m = Fn.nc_std_local(x, w, graph, act, drop, logit_dtype=torch.bfloat16 if form == "one_node_bf16" else torch.float32)
        m.backward(g)
    return step


# the two std calls on prepared tables
with torch.no_grad():
    PQ32 = x.detach() @ torch.cat([w.detach()[:H], w.detach()[H:]], 1)
tables = {"fp32": PQ32, "bf16": Fn.rows_to_bf16(PQ32)}
gPQ = torch.empty((N, 2 * H), device=dev)
gx = torch.empty((N, H), device=dev)
state = {}


def fwd(tag):
    PQ = tables[tag]
    return lambda: state.__setitem__(tag, Fn.nc_std_fwd_launch(x.detach(), PQ[:, :H], PQ[:, H:], graph, act, drop, True))


def bwd(tag):
    PQ = tables[tag]
    return lambda: Fn.nc_std_bwd_launch(x.detach(), PQ[:, :H], PQ[:, H:], g, state[tag][1], graph, act, drop, gPQ[:, :H], gPQ[:, H:], gx)


work = {"step_fp32": (layer_step(layers["fp32"]), args.steps), "step_bf16": (layer_step(layers["bf16"]), args.steps)}
for form in ("two_mm_fp32", "one_node_fp32", "one_node_bf16"):
    work["std_node_" + form] = (node_step(form), args.steps)
for tag in ("fp32", "bf16"):
    work["nc_std_fwd_" + tag] = (fwd(tag), args.reps)
    work["nc_std_bwd_" + tag] = (bwd(tag), args.reps)

for name, (fn, n) in work.items():           # warm-up: plans, allocator, code objects; the forward before its backward
    for _ in range(args.warmup):
        fn()
torch.cuda.synchronize()
ms = {name: [] for name in work}
for _ in range(args.rounds):                  # interleaved: a drifting clock or a busy neighbour hits both sides alike
    for name, (fn, n) in work.items():
        ms[name].append(timed(fn, n))
med = {name: statistics.median(v) for name, v in ms.items()}
ratio = lambda a, b: round(med[a] / med[b], 4)
out = {"device": torch.cuda.get_device_name(0), "N": N, "E": E, "H": H, "K": 1, "activation": args.activation, "dropout": args.dropout, "rounds": args.rounds,
       "steps": args.steps, "reps": args.reps, "median_ms": {k: round(v, 4) for k, v in med.items()},
       "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
       "bf16_over_fp32": dict(nc_std_fwd=ratio("nc_std_fwd_bf16", "nc_std_fwd_fp32"), nc_std_bwd=ratio("nc_std_bwd_bf16", "nc_std_bwd_fp32"),
                              std_node=ratio("std_node_one_node_bf16", "std_node_two_mm_fp32"), step=ratio("step_bf16", "step_fp32")),
       "one_node_fp32_over_two_mm_fp32": ratio("std_node_one_node_fp32", "std_node_two_mm_fp32")}
print(json.dumps(out))
