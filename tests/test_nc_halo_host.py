"""CPU-side tests (-m "not gpu") of what the eight NC entry points (mma_nc_fused_fwd / _bwd, mma_nc_std_fwd / _bwd and their bf16-table
`_h` twins; include/mma_amd.h) refuse of the HALO form's own arguments on the host, before any launch: a drop_edge_base outside
[0, 2^32 - E) (make_drop, csrc/nc_shared.h: edge position + base is a 32-bit key), and in the backward a number of targets beyond the
number of source rows.  The argument sets are those of test_nc_bf16_host.py and test_nc_std_bf16_host.py, all valid until one is changed."""
import pytest

import test_nc_bf16_host as fused
import test_nc_std_bf16_host as std

ENTRIES = [(m, name) for m in (fused, std) for twins in m.TWINS for name in twins]
BACKWARD = [(m, twins) for m in (fused, std) for twins in m.TWINS if twins[0].endswith("_bwd")]
ids = lambda v: v if isinstance(v, str) else ("-".join(v) if isinstance(v, tuple) else "")


def test_all_eight_entry_points_are_covered():
    assert sorted(name for _, name in ENTRIES) == sorted(
        "mma_nc_%s_%s%s" % (k, d, h) for k in ("fused", "std") for d in ("fwd", "bwd") for h in ("", "_h"))
    assert [t for _, t in BACKWARD] == [("mma_nc_fused_bwd", "mma_nc_fused_bwd_h"), ("mma_nc_std_bwd", "mma_nc_std_bwd_h")]
    assert fused.E == std.E == 4


@pytest.mark.parametrize("drop_mode", [0, 1], ids=["NONE", "HASH"])            # the check is unconditional: with no dropout as well
@pytest.mark.parametrize("base", [-1, 2 ** 32 - 4, 2 ** 32, 2 ** 40], ids=["minus1", "2p32-E", "2p32", "2p40"])
@pytest.mark.parametrize("m,name", ENTRIES, ids=ids)
def test_a_drop_edge_base_out_of_range_is_refused(m, name, base, drop_mode):
    assert base < 0 or base + m.E >= 2 ** 32
    got = m._refusal(name, drop_edge_base=base, drop_mode=drop_mode, drop_thr=32768 if drop_mode else 0)
    assert "drop_edge_base %d out of range" % base in got, got
    twin = name[:-2] if name.endswith("_h") else name + "_h"
    assert got == m._refusal(twin, drop_edge_base=base, drop_mode=drop_mode, drop_thr=32768 if drop_mode else 0)


@pytest.mark.parametrize("m,name", ENTRIES, ids=ids)
def test_the_largest_drop_edge_base_passes_the_host_checks(m, name):
    """2^32 - 1 - E is accepted: with it the same call is refused only for what is wrong NEXT (an unknown drop_mode, which make_drop checks
    right after the base)."""
    got = m._refusal(name, drop_edge_base=2 ** 32 - 1 - m.E, drop_mode=7)
    assert "drop_mode 7 unknown" in got and "drop_edge_base" not in got, got


@pytest.mark.parametrize("m,twins", BACKWARD, ids=ids)
def test_more_targets_than_source_rows_are_refused(m, twins):
    f32, h = twins
    got = m._refusal(h, n_targets=m.N + 1)
    assert got == m._refusal(f32, n_targets=m.N + 1)                            # the same check, the same text
    assert "n_targets" in got and ("<= N" in got), got
    assert "n_targets" in m._refusal(h, n_targets=-1)


@pytest.mark.parametrize("name", std.TWINS[1])
def test_the_std_backward_refuses_no_targets(name):
    got = std._refusal(name, n_targets=0)                                      # its node pass has nothing to launch on
    assert "n_targets=0: 1 <= n_targets <= N=%d" % std.N in got, got
