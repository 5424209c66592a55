"""End-to-end smoke of the model glue on the HIP path: the reference's two training loops
(node_classification/train.py:72-96, graph_regression/mma.py:139-161) on small synthetic data - the loss must go down.
Not a parity test (the reference's always-on dropout makes training stochastic); it proves the drop-in modules train."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_node_classification_training_loop():
    from mma_amd.models import MMAConv
    from mma_amd.utils import accuracy, sparse_mx_to_torch_sparse_tensor
    import scipy.sparse as sp
    rng = np.random.default_rng(0)
    N, C, nfeat = 600, 3, 32
    labels = rng.integers(0, C, N)
    same = labels[:, None] == labels[None, :]
    a = (rng.random((N, N)) < np.where(same, 0.03, 0.002))
    a = np.triu(a, 1); a = a | a.T
    for i in np.nonzero(a.sum(1) == 0)[0]:                 # the reference needs degree >= 1 (Q12)
        j = (i + 1) % N; a[i, j] = a[j, i] = True
    adj_sp = sp.csr_matrix(a.astype(np.float32))
    add_all = [adj_sp.indices[adj_sp.indptr[i]:adj_sp.indptr[i + 1]] for i in range(N)]
    feats = (np.eye(C)[labels] @ rng.standard_normal((C, nfeat)) + rng.standard_normal((N, nfeat))).astype(np.float32)
    torch.manual_seed(42)
    model = MMAConv(add_all, "new_sigmoid", 2, nfeat, 16, C, 0.5, ["mean", "max", "min"], DEV).to(DEV)
    adj = sparse_mx_to_torch_sparse_tensor(adj_sp).to(DEV)
    x, y = torch.from_numpy(feats).to(DEV), torch.from_numpy(labels).to(DEV)
    idx_train = torch.arange(0, 400, device=DEV); idx_val = torch.arange(400, 600, device=DEV)
    opt = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=5e-4)
    losses = []
    for epoch in range(60):
        model.train(); opt.zero_grad()
        out = model(x, adj)
        loss = F.nll_loss(out[idx_train], y[idx_train])
        loss.backward(); opt.step()
        losses.append(loss.item())
    model.eval()
    with torch.no_grad():
        acc = accuracy(model(x, adj)[idx_val], y[idx_val]).item()
    assert np.isfinite(losses).all() and np.mean(losses[-5:]) < 0.6 * np.mean(losses[:5]), losses[::10]
    assert acc > 0.55, acc          # chance is 0.33
    assert len(list(model.parameters())) == 25      # weight0,bias0,weight1,bias1 + 21 masks, as models.py:45-50


def test_graph_regression_training_loop():
    from mma_amd.net import Net
    from test_gr_gpu import molecule_batch
    rng = np.random.default_rng(1)
    batches = []
    for _ in range(4):
        ei, N, sizes = molecule_batch(rng, 16, return_sizes=True)
        comp = np.repeat(np.arange(16), sizes)                  # the `batch` vector of a PyG mini-batch
        xt = rng.integers(0, 21, (N, 1))
        et = rng.integers(1, 4, ei.shape[1])
        yv = np.bincount(comp, weights=(xt[:, 0] % 5).astype(np.float64), minlength=16) / 10.0
        batches.append((torch.from_numpy(xt).to(DEV), torch.from_numpy(ei).to(DEV), torch.from_numpy(et).to(DEV),
                        torch.from_numpy(comp).to(DEV), torch.from_numpy(yv.astype(np.float32)).to(DEV)))
    deg = torch.zeros(5, dtype=torch.long)
    for _, ei, _, comp, _ in batches:
        d = torch.bincount(ei[1].cpu(), minlength=comp.numel())
        deg += torch.bincount(d, minlength=5)[:5]
    torch.manual_seed(0)
    model = Net(["min", "max"], ["identity", "amplification", "linear"], deg).to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=0.003)
    hist = []
    for epoch in range(25):
        tot = 0.0
        for xt, ei, et, comp, yv in batches:
            opt.zero_grad()
            out = model(xt, ei, et, comp)
            loss = (out.squeeze() - yv).abs().mean()
            loss.backward(); opt.step()
            tot += loss.item()
        hist.append(tot / len(batches))
    assert np.isfinite(hist).all() and np.mean(hist[-3:]) < 0.7 * np.mean(hist[:3]), hist[::5]


@pytest.mark.gpu
def test_bench_default_run_ends_with_one_compact_strict_metric_line():
    """Round-4 VERDICT item 1, on the real thing: `python bench.py --full` (C4, secondary configs, CPU baselines) - the
    LAST stdout line strict-parses, is < 4096 bytes and carries roofline.frac and cpu_baseline.value; the verbose record is on stderr."""
    import subprocess
    import sys
    from bench_util import parse_bench
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2", "--full"], capture_output=True, text=True, timeout=900,
                       env=env, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    d, det = parse_bench(r, need_cpu=True)
    assert d["n_gpus"] == 1 and d["steps"] == 5 and d["warmup"] == 2 and d["config"]["edges"] > 10_000_000 and d["dtype"] == "f32"
    assert d["roofline"]["kernel"] in ("nc_fused_fwd", "nc_fused_bwd") and d["roofline"]["frac"] > 0.5
    assert set(det["extra"]) >= {"C1", "C3", "C2", "C2L", "C5shard"} and not any("error" in v for v in det["extra"].values()), det["extra"]
    assert abs(d["value"] - d["config"]["edges"] / d["ms_per_step"] * 1e3) <= 1e-3 * d["value"]


@pytest.mark.gpu
def test_bench_c2l_line_is_compact_strict_and_names_the_fused_gr_kernel():
    """`python bench.py --workload c2l --full` (the graph-regression leg): the same contract for its line - one strict-JSON line < 4096 bytes with
    `roofline` (K3 / K4 by their algorithmic bytes) and `cpu_baseline` (the GR oracle on a small batch); the per-call table is on stderr."""
    import subprocess
    import sys
    from bench_util import parse_bench
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, "bench.py", "--workload", "c2l", "--molecules", "2000", "--steps", "3", "--warmup", "1", "--full"], capture_output=True,
                       text=True, timeout=600, env=env, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    d, det = parse_bench(r, need_cpu=True)
    assert d["scaling"] == "weak" and d["roofline"]["kernel"] in ("gr_fused_fwd", "gr_fused_bwd") and d["roofline_other"]["kernel"].startswith("gr_fused")
    assert {"gr_fused_fwd", "gr_fused_bwd", "gr_segsum", "tower_post_gw"} <= set(det["kernels"]) and det["kernels"]["gr_fused_fwd"]["bytes"] > 0


@pytest.mark.gpu
def test_bench_plain_run_is_lean_and_its_dumped_outputs_repeat(tmp_path):
    """A plain `python bench.py` times exactly --steps steps and does nothing the headline does not need (no CPU baseline, no plan-build
    timing, no secondary configs); --dump-outputs writes what its last step computed, and two runs with the same arguments write the
    same arrays."""
    import subprocess
    import sys
    from bench_util import parse_bench
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    dumps = []
    for run in range(2):
        out = tmp_path / ("run%d" % run)
        r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "4", "--warmup", "1", "--scale", "15", "--edges", "150000",
                            "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, env=env, cwd=root)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        d, det = parse_bench(r)
        assert d["steps"] == 4 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["dtype"] == "f32"
        assert abs(d["value"] - d["config"]["edges"] / d["ms_per_step"] * 1e3) <= 1e-3 * d["value"]
        assert d["cpu_baseline"] is None and det["extra"] is None and det["plan_build"] is None
        assert det["kernels"]["nc_fused_fwd"]["launches"] >= 4
        dumps.append({f.name[:-4]: np.load(f) for f in sorted(out.glob("*.npy"))})
    a, b = dumps
    N = a["grad_x"].shape[0]
    assert {"out", "grad_x", "sample_rows", "grad_weight", "grad_bias", "grad_mask_sum", "grad_mask_min"} <= set(a) and set(a) == set(b)
    assert a["out"].shape == (N, 16) and a["grad_x"].shape == (N, 128) and a["grad_mask_max"].shape == (256, 128)
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for k in a:
        np.testing.assert_allclose(b[k], a[k], rtol=1e-5, atol=1e-6 * max(1.0, float(np.abs(a[k]).max())), err_msg=k)
