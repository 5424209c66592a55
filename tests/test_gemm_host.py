"""CPU-side tests (-m "not gpu") of what the fp32 GEMM entry points of mma_amd/csrc/gemm_x3.hip refuse on the host, before any launch:
CPU tensors through _lib.call, each refusal matched against its text.  Nothing here launches: every call is either refused, or has
M == 0 / n == 0 and returns before a pointer is looked at.  The workspace queries are pinned at the plans tests/test_gemm_edges_gpu.py
relies on (an empty split, the plan change at 65 536 rows, the batched plan), so those numbers hold where no GPU is needed.
The three bf16-output twins have their own file (tests/test_gemm_bf16_out_host.py)."""
import os
import re

import pytest
import torch

from mma_amd import _lib

from gemm_ref import hip_entry_points

M, N, K = 8, 128, 256
HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mma_amd", "csrc", "gemm_x3.hip")

f = lambda *s: torch.zeros(*s, dtype=torch.float32)
NN = ("mma_gemm_bf16x3", "mma_gemm_f16x2", "mma_gemm_f16x2_k", "mma_gemm_f16x2_k256", "mma_gemm_f16x2_k256p", "mma_gemm_f16x2_n128",
      "mma_gemm_f16x2_nlp")
TN = ("mma_gemm_bf16x3_tn", "mma_gemm_f16x2_tn", "mma_gemm_bf16x3_tn_batched")
K_OF = {"mma_gemm_bf16x3": 256, "mma_gemm_f16x2": 128, "mma_gemm_f16x2_k": 64, "mma_gemm_f16x2_k256": 256, "mma_gemm_f16x2_k256p": 256,
        "mma_gemm_f16x2_n128": 192, "mma_gemm_f16x2_nlp": 256}


def _values(name):
    """Well-formed arguments of every entry point, by parameter name (CPU tensors: only calls that stop on the host are made)."""
    k = K_OF.get(name, K)
    v = dict(A=f(M, k), lda=k, Bt3=torch.zeros(3, N, k, dtype=torch.bfloat16), Bt2=torch.zeros(2, N, k, dtype=torch.float16), C=f(M, N), ldc=N,
             col_unscale=f(N), a_row_max=None, row_max=f(M), Ap=torch.zeros(32 * 1024, dtype=torch.uint8), sce=torch.zeros(M, dtype=torch.int32),
             M=M, N=N, K=k, accumulate=0, stream=None)
    v["in"] = f(16)
    v.update(n=16, out_3n_bf16=torch.zeros(48, dtype=torch.bfloat16), out=f(M), cols=k)
    if name in TN:
        ka, nc, b = 32, 32, 2
        v.update(X=f(64, 64), ldx=64, xb=ka, G=f(64, 64), ldg=64, gb=nc, C=f(b * ka * nc), ws=f(1 << 16), ws_floats=1 << 16, M=64, KA=ka,
                 NC=nc, B=b, x_row_max=f(64), g_row_max=f(64))
    return v


def _args(name, **over):
    vals = _values(name)
    vals.update(over)
    return [vals[n] for _, _, n in _lib._abi.FUNCTIONS[name][1]]


def _refusal(name, **over):
    with pytest.raises(_lib.MMALibraryError) as e:
        _lib.call(name, *_args(name, **over))
    return str(e.value)


def _off(t, nbytes):
    """A view of t's storage nbytes further on (a misaligned pointer)."""
    raw = torch.zeros(t.numel() * t.element_size() + 64, dtype=torch.uint8)
    assert raw.data_ptr() % 16 == 0
    return raw[nbytes:]


def test_the_file_defines_the_entry_points_these_tests_name():
    names = hip_entry_points(HIP)
    assert set(NN) | set(TN) | {"mma_split_bf16x3", "mma_split_f16x2", "mma_row_absmax", "mma_pack_f16x2_k256", "mma_pack_f16x2_k256_bytes",
                                "mma_gemm_bf16x3_tn_workspace_floats", "mma_gemm_bf16x3_tn_batched_workspace_floats",
                                "mma_gemm_f16x2_tn_workspace_floats", "mma_gemm_f16x2_k_h", "mma_gemm_f16x2_k256_h", "mma_gemm_f16x2_k256p_h"} == set(names)
    assert all(n in _lib._abi.FUNCTIONS for n in names)


# ---- shape rules ----------------------------------------------------------------------------------------------------------------------------
SHAPES = [
    ("mma_gemm_bf16x3", dict(N=48, ldc=48), r"need N % 32 == 0, K % 128 == 0"),
    ("mma_gemm_bf16x3", dict(N=0, ldc=32), r"need N % 32 == 0"),
    ("mma_gemm_bf16x3", dict(K=192, lda=192), r"M=8 N=128 K=192: need N % 32 == 0, K % 128 == 0"),
    ("mma_gemm_bf16x3", dict(K=64, lda=64), r"K % 128 == 0"),
    ("mma_gemm_bf16x3", dict(M=-1), r"M=-1"),
    ("mma_gemm_bf16x3", dict(K=256, N=160, ldc=160), r"either K == 128 or N <= 128"),
    ("mma_gemm_f16x2", dict(N=192, ldc=192), r"need N % 128 == 0, N <= 4096"),
    ("mma_gemm_f16x2", dict(N=4224, ldc=4224), r"N <= 4096"),
    ("mma_gemm_f16x2_k", dict(K=80, lda=80), r"K=80 unsupported \(64, 96 or 128\)"),
    ("mma_gemm_f16x2_k", dict(K=32, lda=32), r"K=32 unsupported"),
    ("mma_gemm_f16x2_k", dict(K=256, lda=256), r"K=256 unsupported"),
    ("mma_gemm_f16x2_k", dict(N=64, ldc=64), r"need N % 128 == 0"),
    ("mma_gemm_f16x2_k256", dict(N=64, ldc=64), r"need N % 128 == 0"),
    ("mma_gemm_f16x2_k256p", dict(N=192, ldc=192), r"need N % 128 == 0"),
    ("mma_gemm_f16x2_n128", dict(K=96, lda=96), r"M=8 K=96: need K % 64 == 0"),
    ("mma_gemm_f16x2_n128", dict(K=0, lda=64), r"need K % 64 == 0"),
    ("mma_gemm_f16x2_n128", dict(M=-3), r"M=-3"),
    ("mma_gemm_f16x2_nlp", dict(N=64, ldc=64), r"need N in \{128, 256\}, K % 128 == 0, K >= 256"),
    ("mma_gemm_f16x2_nlp", dict(N=384, ldc=384), r"need N in \{128, 256\}"),
    ("mma_gemm_f16x2_nlp", dict(K=128, lda=128), r"K >= 256"),
    ("mma_gemm_f16x2_nlp", dict(K=320, lda=320), r"M=8 N=128 K=320: need N in \{128, 256\}, K % 128 == 0"),
    ("mma_gemm_bf16x3_tn", dict(KA=0), r"need 1 <= KA <= 128, NC >= 1"),
    ("mma_gemm_bf16x3_tn", dict(KA=129, ldx=256), r"KA=129 NC=32: need 1 <= KA <= 128"),
    ("mma_gemm_bf16x3_tn", dict(NC=0), r"NC >= 1"),
    ("mma_gemm_bf16x3_tn", dict(M=0), r"M=0 KA=32"),
    ("mma_gemm_f16x2_tn", dict(KA=257, ldx=512), r"need M < 2\^30, 1 <= KA <= 256, NC >= 1"),
    ("mma_gemm_f16x2_tn", dict(KA=0), r"1 <= KA <= 256"),
    ("mma_gemm_f16x2_tn", dict(M=0), r"M=0"),
    ("mma_gemm_f16x2_tn", dict(M=1 << 30), r"M=1073741824 KA=32 NC=32: need M < 2\^30"),
    ("mma_gemm_bf16x3_tn_batched", dict(B=0), r"B=0: need 1 <= KA <= 128, NC >= 1, 1 <= B <= 65535"),
    ("mma_gemm_bf16x3_tn_batched", dict(B=65536, xb=0, gb=0), r"B=65536"),
    ("mma_gemm_bf16x3_tn_batched", dict(KA=129), r"1 <= KA <= 128"),
    ("mma_gemm_bf16x3_tn_batched", dict(M=0), r"M=0"),
    ("mma_gemm_bf16x3_tn_batched", dict(B=3), r"the B column blocks do not fit the row pitch"),             # 2 * 32 + 32 > 64
    ("mma_gemm_bf16x3_tn_batched", dict(gb=40), r"the B column blocks do not fit the row pitch"),            # 40 + 32 > 64
    ("mma_gemm_bf16x3_tn_batched", dict(xb=-1), r"NULL argument, or the B column blocks do not fit"),
    ("mma_split_bf16x3", dict(n=-1), r"n < 0"),
    ("mma_split_f16x2", None, r"K=0 N=128 out of range"),
    ("mma_row_absmax", dict(cols=0), r"cols=0 lda=256 out of range"),
    ("mma_row_absmax", dict(lda=K - 1), r"out of range"),
    ("mma_row_absmax", dict(lda=1 << 24), r"out of range"),
    ("mma_pack_f16x2_k256", dict(lda=252), r"need lda >= 256, lda % 4 == 0"),
    ("mma_pack_f16x2_k256", dict(lda=258), r"lda=258: need lda >= 256, lda % 4 == 0"),
    ("mma_pack_f16x2_k256", dict(M=-1), r"M=-1"),
]


@pytest.mark.parametrize("name,over,text", SHAPES, ids=["%02d-%s" % (i, s[0][4:]) for i, s in enumerate(SHAPES)])
def test_shape_rules(name, over, text):
    if name == "mma_split_f16x2":
        with pytest.raises(_lib.MMALibraryError, match=text):
            _lib.call(name, f(4, N), N, 1, 0, N, torch.zeros(2, N, 4, dtype=torch.float16), f(N), 0, None)
        return
    got = _refusal(name, **over)
    assert re.search(text, got), got


# ---- pitches and pointers --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in NN if n != "mma_gemm_f16x2_k256p"])
def test_nn_entries_refuse_bad_pitches_of_a(name):
    k = K_OF[name]
    for over in (dict(lda=k - 4), dict(lda=k + 2), dict(lda=1 << 24)):                 # narrower than K, no whole float4s, >= 2^24
        assert "row pitch too small, unaligned or >= 2^24" in _refusal(name, **over), over


@pytest.mark.parametrize("name", NN)
def test_nn_entries_refuse_bad_pitches_of_c(name):
    for over in (dict(ldc=N - 1), dict(ldc=1 << 24)):
        assert "row pitch too small" in _refusal(name, **over), over


@pytest.mark.parametrize("name", NN)
def test_nn_entries_refuse_null_and_misaligned_pointers(name):
    params = [n for _, _, n in _lib._abi.FUNCTIONS[name][1]]
    for p in params:
        if p in ("A", "Ap", "Bt2", "Bt3", "C", "col_unscale", "row_max", "sce"):
            assert "NULL or misaligned argument" in _refusal(name, **{p: None}), p
    for p in ("A", "Ap", "Bt2", "Bt3"):                                                 # 16-byte alignment: 4 bytes off is refused
        if p in params:
            assert "NULL or misaligned argument" in _refusal(name, **{p: _off(_values(name)[p], 4)}), p


@pytest.mark.parametrize("name", NN + ("mma_row_absmax", "mma_pack_f16x2_k256"))
def test_nothing_to_do_returns_before_any_pointer_is_looked_at(name):
    """M == 0 returns 0 ahead of the pointer checks (the comment above nn_operands): every pointer NULL, no launch, no error."""
    nulls = {n: None for k, _, n in _lib._abi.FUNCTIONS[name][1] if k == "T"}
    assert _lib.call(name, *_args(name, M=0, **nulls)) is None
    # ... but a bad shape or pitch is still refused at M == 0
    if name in NN:
        assert "row pitch too small" in _refusal(name, M=0, ldc=N - 1)


def test_split_bf16x3_of_nothing_is_no_error_and_null_is_refused():
    assert _lib.call("mma_split_bf16x3", None, 0, None, None) is None
    assert "NULL argument" in _refusal("mma_split_bf16x3", out_3n_bf16=None)
    with pytest.raises(_lib.MMALibraryError, match="NULL argument"):
        _lib.call("mma_split_f16x2", None, N, 1, 4, N, torch.zeros(2, N, 4, dtype=torch.float16), f(N), 0, None)
    with pytest.raises(_lib.MMALibraryError, match="strides out of range"):
        _lib.call("mma_split_f16x2", f(4, N), -1, 1, 4, N, torch.zeros(2, N, 4, dtype=torch.float16), f(N), 0, None)


def test_row_absmax_and_pack_refuse_null_and_misaligned():
    assert "NULL or misaligned argument" in _refusal("mma_row_absmax", A=None)
    assert "NULL or misaligned argument" in _refusal("mma_row_absmax", out=None)
    assert "NULL or misaligned argument" in _refusal("mma_row_absmax", A=_off(f(M, K), 2))              # 4-byte alignment
    for p in ("A", "Ap", "sce"):
        assert "NULL or misaligned argument" in _refusal("mma_pack_f16x2_k256", **{p: None}), p
    assert "NULL or misaligned argument" in _refusal("mma_pack_f16x2_k256", A=_off(f(M, K), 4))
    assert "NULL or misaligned argument" in _refusal("mma_pack_f16x2_k256", Ap=_off(torch.zeros(32 * 1024, dtype=torch.uint8), 8))


@pytest.mark.parametrize("name", TN)
def test_tn_entries_refuse_pitches_and_pointers(name):
    text = "NULL argument" if name != "mma_gemm_bf16x3_tn_batched" else "NULL argument, or the B column blocks"
    for over in (dict(X=None), dict(G=None), dict(C=None), dict(ldx=31), dict(ldg=31), dict(ldx=1 << 24), dict(ldg=1 << 24)):
        got = _refusal(name, **over)
        assert text in got and ("row pitch" in got), (over, got)
    for over in (dict(X=_off(f(64, 64), 2)), dict(G=_off(f(64, 64), 2))):                                # 4-byte alignment of X and G
        assert "misaligned argument" in _refusal(name, **over), over
    if name == "mma_gemm_f16x2_tn":
        assert "NULL argument" in _refusal(name, ws=None)                                                # never NULL for this form
        assert "misaligned argument" in _refusal(name, ws=_off(f(1 << 16), 4))                           # 16-byte alignment of ws


# ---- workspaces and the 2 GB window --------------------------------------------------------------------------------------------------------------
def _ws(name, *a):
    return _lib.query(name, *a)


def test_workspace_too_small_names_the_needed_count():
    Mt, ka, nc = 4096, 32, 32
    need = _ws("mma_gemm_bf16x3_tn_workspace_floats", Mt, ka, nc)
    assert need > 0 and need % (ka * nc) == 0
    big = dict(X=f(8, 64), G=f(8, 64), M=Mt)                    # (refused before a row is read)
    got = _refusal("mma_gemm_bf16x3_tn", ws_floats=need - 1, **big)
    assert "workspace too small: %d floats, need %d" % (need - 1, need) in got
    assert "workspace too small: 0 floats, need %d" % need in _refusal("mma_gemm_bf16x3_tn", ws=None, ws_floats=0, **big)
    need2 = _ws("mma_gemm_f16x2_tn_workspace_floats", Mt, ka, nc)
    assert "workspace too small: %d floats, need %d" % (need2 - 1, need2) in _refusal("mma_gemm_f16x2_tn", ws_floats=need2 - 1, **big)
    need3 = _ws("mma_gemm_bf16x3_tn_batched_workspace_floats", Mt, ka, nc, 2)
    assert need3 > 0
    assert "workspace too small: %d floats, need %d" % (need3 - 1, need3) in _refusal("mma_gemm_bf16x3_tn_batched", ws_floats=need3 - 1, **big)


@pytest.mark.parametrize("name", TN)
def test_row_range_of_one_split_must_fit_a_2gb_window(name):
    """(rows of one split + one 32-row chunk) * pitch * 4 bytes must stay below 2^31: the smallest pitch that does not is refused (it is
    still a legal pitch, < 2^24).  The split count is the library's own."""
    from gemm_ref import tn_rows_per_split, tn_splits, tn_splits_batched
    splits = tn_splits_batched(64, 32, 32, 2) if name == "mma_gemm_bf16x3_tn_batched" else tn_splits(64, 32, 32)
    pitch = -(-(1 << 31) // ((tn_rows_per_split(64, splits) + 32) * 4))
    assert pitch < 1 << 24
    over = dict(ldx=pitch) if name != "mma_gemm_bf16x3_tn_batched" else dict(ldg=pitch)
    assert "row range of one split exceeds a 2 GB buffer window" in _refusal(name, **over)


def test_workspace_queries_return_0_for_non_positive_sizes():
    for a in ((0, 32, 32), (-1, 32, 32), (64, 0, 32), (64, 32, 0), (64, -5, 32)):
        assert _ws("mma_gemm_bf16x3_tn_workspace_floats", *a) == 0
        assert _ws("mma_gemm_f16x2_tn_workspace_floats", *a) == 0
        assert _ws("mma_gemm_bf16x3_tn_batched_workspace_floats", *a, 2) == 0
    assert _ws("mma_gemm_bf16x3_tn_batched_workspace_floats", 64, 32, 32, 0) == 0
    assert _ws("mma_pack_f16x2_k256_bytes", 0) == 0 and _ws("mma_pack_f16x2_k256_bytes", -7) == 0
    assert _ws("mma_pack_f16x2_k256_bytes", 1) == 32 * 1024 and _ws("mma_pack_f16x2_k256_bytes", 33) == 64 * 1024


def test_workspace_queries_reproduce_the_plans_the_gpu_tests_rely_on():
    from gemm_ref import tn_rows_per_split, tn_splits, tn_splits_batched
    # (128, 32, 32): 3 splits of 64 rows - the third starts at row 128 and is empty; one more row gives it one
    assert tn_splits(128, 32, 32) == 3 and tn_rows_per_split(128, 3) == 64
    assert tn_splits(129, 32, 32) == 3 and tn_rows_per_split(129, 3) == 64
    assert tn_splits(1, 32, 32) == 1 and tn_splits(63, 32, 32) == 1 and tn_splits(64, 32, 32) == 2
    # the plan change: 2 chunks of 32 rows per split at least below 65 536 rows, 8 from there on
    assert tn_splits(65535, 32, 32) == 512 and tn_rows_per_split(65535, 512) == 128
    assert tn_splits(65536, 32, 32) == 256 and tn_rows_per_split(65536, 256) == 256
    # the batch of the post-NN weight gradients at 4 096 + 33 rows: 16 splits of 288 rows, the last one empty
    assert tn_splits_batched(4129, 48, 152, 5) == 16 and tn_rows_per_split(4129, 16) == 288 and 15 * 288 >= 4129
    assert tn_splits_batched(4129, 48, 152, 1) == 16 and tn_splits_batched(4129, 8, 32, 2) == 16


@pytest.mark.parametrize("Mt,ka", [(1, 1), (33, 33), (1000, 100), (65536, 200), (70001, 256)])
def test_packx_enlarges_the_f16x2_tn_workspace_by_one_4kb_block_per_chunk_and_column_block(Mt, ka, monkeypatch):
    nc = 300
    monkeypatch.setenv("MMA_TN_PACKX", "0")
    plain = _ws("mma_gemm_f16x2_tn_workspace_floats", Mt, ka, nc)
    monkeypatch.setenv("MMA_TN_PACKX", "1")
    packed = _ws("mma_gemm_f16x2_tn_workspace_floats", Mt, ka, nc)
    assert packed - plain == -(-Mt // 32) * -(-ka // 32) * 1024
    six = _ws("mma_gemm_bf16x3_tn_workspace_floats", Mt, ka, nc)
    assert plain == -(-six // 4) * 4 + 3 * (-(-Mt // 32) * 32) + 4          # partial tiles | row maxima of X, of G | scale halves | state
