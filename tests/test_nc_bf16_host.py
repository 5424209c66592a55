"""CPU-side tests (-m "not gpu") of the bf16 logit-table entry points (include/mma_amd.h ABI 38: mma_nc_fused_fwd_h, mma_nc_fused_bwd_h,
mma_rows_to_bf16) and of the `logit_dtype` keyword: every bad argument the fp32 entry points refuse on the host is refused by their
bf16 twins with the same text, before any launch - no GPU is needed to see it."""
import re

import pytest
import torch

from mma_amd import _lib
from mma_amd import functional as Fn

N, E, H, K = 4, 4, 4, 2
KINDS, ACTS = [0, 2], [0, 1]                       # sum, max: one code slot -> crow rows of 8 floats
LDC = 8
TWINS = [("mma_nc_fused_fwd", "mma_nc_fused_fwd_h"), ("mma_nc_fused_bwd", "mma_nc_fused_bwd_h")]


def _values(table_dtype):
    f = lambda *s: torch.zeros(*s, dtype=torch.float32)
    i = lambda *s: torch.zeros(*s, dtype=torch.int32)
    t = lambda *s: torch.zeros(*s, dtype=table_dtype)
    KH = K * H
    return dict(
        x=f(N, H), ldx=H, P=t(N, KH), ldp=KH, Q=t(N, KH), ldq=KH, rowptr=i(N + 1), col=i(E), items=i(N, 4), n_items=N, n_wave_items=N,
        hubs=None, n_hubs=0, partial=None, n_slots=0, m=None, m_sum=f(N, H), ldms=H, T=f(N, KH), sel=None, ldt=KH, crow=f(N, LDC), ldc=LDC,
        N=N, E=E, H=H, K=K, kind_host=KINDS, act_host=ACTS, drop_mode=0, drop_thr=0, seed=0, seed_dev=None, drop_edge_base=0, keep=None,
        sync=None, stream=None,
        # the backward's own
        gs=None, ldg=KH, g=f(N, H), ldgg=H, gxs=None, ldgx=H, gP=f(N, KH), ldgp=KH, n_targets=N, t_col=i(E), t_eid=i(E),
        gQ=f(N, KH), ldgq=KH, gx=f(N, H), ldgxo=H, row_max=None)


def _args(name, **over):
    vals = _values(torch.bfloat16 if name.endswith("_h") else torch.float32)
    vals.update(over)
    return [vals[n] for _, _, n in _lib._abi.FUNCTIONS[name][1]]


def _refusal(name, **over):
    with pytest.raises(_lib.MMALibraryError) as e:
        _lib.call(name, *_args(name, **over))
    return str(e.value).replace(name, "<entry>")


def test_the_new_entry_points_are_declared():
    for name in ("mma_nc_fused_fwd_h", "mma_nc_fused_bwd_h", "mma_rows_to_bf16"):
        assert name in _lib._abi.FUNCTIONS and name in _lib.PROTOTYPES
    for f32, h in TWINS:             # same parameter lists: only the storage of P and Q differs (the bindings see both as pointers)
        assert _lib._abi.FUNCTIONS[f32] == _lib._abi.FUNCTIONS[h]
    assert [n for _, _, n in _lib._abi.FUNCTIONS["mma_rows_to_bf16"][1]] == ["src", "lds", "dst", "ldd", "rows", "cols", "stream"]
    assert _lib.ABI_VERSION >= 38


BAD = [
    (dict(N=-1), "out of int32 range"),
    (dict(E=-3), "out of int32 range"),
    (dict(H=0), "H=0 K=2 unsupported"),
    (dict(K=9, kind_host=[0] * 9, act_host=[0] * 9), "K=9 unsupported"),
    (dict(ldp=K * H - 1), "pitch too small"),
    (dict(ldq=H), "pitch too small"),
    (dict(ldx=2), "pitch too small"),
    (dict(ldp=1 << 31), "pitch out of range"),
    (dict(n_items=-1), "negative or oversize item counts"),
    (dict(n_slots=3), "hub slots without"),
    (dict(items=None), "NULL argument"),
    (dict(P=None), "NULL argument"),
    (dict(act_host=[0, 5]), r"act\[1\]=5"),
    (dict(kind_host=[9, 0]), r"kind\[0\]=9"),
    (dict(drop_mode=2), "keep mask"),
    (dict(drop_mode=7), "drop_mode 7 unknown"),
]


@pytest.mark.parametrize("f32,h", TWINS)
@pytest.mark.parametrize("over,text", BAD, ids=["%d-%s" % (n, "-".join(sorted(o))) for n, (o, _) in enumerate(BAD)])
def test_h_entry_points_refuse_what_their_fp32_twins_refuse(f32, h, over, text):
    assert len(_args(h)) == len(_lib.PROTOTYPES[h])
    want, got = _refusal(f32, **over), _refusal(h, **over)
    assert got == want                                      # the same check, the same text
    assert re.search(text, got), got


@pytest.mark.parametrize("f32,h", TWINS)
def test_h_entry_points_refuse_misaligned_item_lists(f32, h):
    base = torch.zeros(12, dtype=torch.int32)
    assert base.data_ptr() % 16 == 0
    over = dict(hubs=base[1:5], n_hubs=1, partial=torch.zeros(64), n_slots=1)                        # 4 bytes off
    assert _refusal(h, **over) == _refusal(f32, **over) and "16-byte aligned" in _refusal(h, **over)


def test_forward_h_refuses_saved_state_without_T():
    over = dict(T=None)                                     # crow given without T
    assert _refusal("mma_nc_fused_fwd_h", **over) == _refusal("mma_nc_fused_fwd", **over)
    assert "give T too" in _refusal("mma_nc_fused_fwd_h", **over)


def test_backward_h_refuses_an_epilogue_without_the_shared_form():
    over = dict(g=None)
    assert _refusal("mma_nc_fused_bwd_h", **over) == _refusal("mma_nc_fused_bwd", **over)
    assert "shared-gradient form" in _refusal("mma_nc_fused_bwd_h", **over)


def test_rows_to_bf16_refuses_bad_arguments():
    src, dst = torch.zeros(3, 8), torch.zeros(3, 8, dtype=torch.bfloat16)
    call = lambda *a: _lib.call("mma_rows_to_bf16", *a, None)
    with pytest.raises(_lib.MMALibraryError, match="out of range"):
        call(src, 8, dst, 8, -1, 8)
    with pytest.raises(_lib.MMALibraryError, match="out of range"):
        call(src, 8, dst, 8, 3, -8)
    with pytest.raises(_lib.MMALibraryError, match="pitch too small"):
        call(src, 8, dst, 4, 3, 8)
    with pytest.raises(_lib.MMALibraryError, match="pitch too small"):
        call(src, 7, dst, 8, 3, 8)
    with pytest.raises(_lib.MMALibraryError, match="NULL argument"):
        call(None, 8, dst, 8, 3, 8)
    with pytest.raises(_lib.MMALibraryError, match="NULL argument"):
        call(src, 8, None, 8, 3, 8)
    call(src, 8, dst, 8, 0, 8)                              # nothing to do: no launch, no error


def _layer(**kw):
    import mma_amd
    from golden.inputs import ALL_MASK_NAMES
    P = lambda *s: torch.nn.Parameter(torch.empty(*s))
    masks = [P(2 * H, H) for _ in ALL_MASK_NAMES]
    return mma_amd.MMA([[1], [0], [], [2]], "sigmoid", 2, H, 3, P(H, 3), P(3), *masks, 0.0, ["sum", "max"], "cpu", **kw)


def test_the_layer_takes_float32_and_bfloat16_only():
    assert _layer().logit_dtype == torch.float32
    assert _layer(logit_dtype=torch.bfloat16).logit_dtype == torch.bfloat16
    assert _layer(logit_dtype=torch.bfloat16, strict_reference=False).logit_dtype == torch.bfloat16      # a storage choice: both modes
    for bad in (torch.float16, torch.float64, "bf16", None):
        with pytest.raises(ValueError, match="logit_dtype"):
            _layer(logit_dtype=bad)
    with pytest.raises(ValueError, match="logit_dtype"):
        Fn.nc_local_layer(torch.zeros(4, 4), torch.zeros(4, 16), None, None, KINDS, ACTS, logit_dtype=torch.float16)


def test_mixed_table_dtypes_raise():
    x, p32, pbf = torch.zeros(N, H), torch.zeros(N, K * H), torch.zeros(N, K * H, dtype=torch.bfloat16)
    for P, Q in ((p32, pbf), (pbf, p32)):
        with pytest.raises(ValueError, match="share a dtype"):
            Fn.nc_fwd_launch(x, P, Q, None, KINDS, ACTS, Fn.DropoutSpec(0.0), True, True)
        with pytest.raises(ValueError, match="share a dtype"):
            Fn.nc_bwd_edges_launch(x, P, Q, None, x, None, None, None, KINDS, ACTS, Fn.DropoutSpec(0.0), None, None, None)
    with pytest.raises(ValueError, match="logit_dtype"):
        Fn.nc_fwd_launch(x, p32.half(), p32.half(), None, KINDS, ACTS, Fn.DropoutSpec(0.0), True, True)
