"""The launch ladder of K3 / K4 (gr_fused.hip: gr_vec4, gr_grid, gr_block_mode, gr_flat_mode, gr_plan) through the host-only query
mma_gr_plan / functional.gr_plan, with no GPU: literal plans on both sides of every gate.  The expected tuples are constants worked out
by hand from the rules of DESIGN.md ("The GR launch ladder"), not recomputed from the library's formula:

    GRPlan(first, vec, nb, needs, lpr_log, chunks, second, lds_bytes)
    first: 0 none, 1 flat, 2 block;  second: 0 none, 1 wave over everything, 2 wave for long segments, 3 list

Block LDS: kBlkHead + nb * D * (4 * planes + 2) <= 40960 with kBlkHead = 2 * 65 * 32 + 32 * 4 + 2 * 256 * 4 + 256 = 6592, i.e.
nb * D * (4 * planes + 2) <= 34368; planes = K forward, 2 ({min, max}) or 3 (with sum / mean) backward."""
import pytest

from mma_amd import _lib
from mma_amd import functional as Fn

SUM, MEAN, MIN, MAX, VAR, STD = range(6)
NONE, FLAT, BLOCK = 0, 1, 2
WAVE, WAVE_LONG, LIST = 1, 2, 3
N0, E0 = 1000, 3000                               # E <= 16 N


def fwd(T=2, F=8, aggr=(MIN, MAX), S=1, N=N0, E=E0, **kw):
    """The plan of a fused forward U + V + Z with dense pitches ([U | V] in one buffer), saved args and the long-node list."""
    D = T * F
    a = dict(lduv=2 * D, ldz=D, ldsave=D, has_z=True, has_list=True)
    a.update(kw)
    return tuple(Fn.gr_plan(N, E, T, F, aggr, tuple(range(S)), **a))


def bwd(T=2, F=8, aggr=(MIN, MAX), S=1, N=N0, E=E0, **kw):
    D = T * F
    a = dict(lduv=2 * D, ldz=D, ldsave=D, ldg=D, ldgu=2 * D, has_z=True, has_list=True, backward=True)
    a.update(kw)
    return tuple(Fn.gr_plan(N, E, T, F, aggr, tuple(range(S)), **a))


def given(T=2, F=8, aggr=(MIN, MAX), S=1, N=N0, E=E0, **kw):
    a = dict(ldi=T * F, ldsave=T * F, given=True, has_list=True)
    a.update(kw)
    return tuple(Fn.gr_plan(N, E, T, F, aggr, tuple(range(S)), **a))


@pytest.fixture(autouse=True)
def no_nb_cap(monkeypatch):
    monkeypatch.delenv("MMA_GR_NB", raising=False)


BASE = (BLOCK, 4, 16, 6, 2, 1, LIST, 9152)         # D = 16: 6592 + 16 * 16 * 10; 4 quads -> 4 lanes per row
FLAT4 = (FLAT, 4, 16, 0, 2, 1, LIST, 0)
FLAT1 = (FLAT, 1, 16, 0, 4, 1, LIST, 0)            # VEC 1 at D = 16: 16 lanes per row


def test_base_plans_and_the_named_tuple():
    p = Fn.gr_plan(N0, E0, 2, 8, (MIN, MAX), (0,), lduv=32, ldz=16, ldsave=16, has_z=True, has_list=True)
    assert p._fields == ("first", "vec", "nb", "needs", "lpr_log", "chunks", "second", "lds_bytes")
    assert tuple(p) == BASE and Fn.GR_FIRST[p.first] == "block" and Fn.GR_SECOND[p.second] == "list"
    assert fwd() == BASE and bwd() == BASE and given() == BASE
    assert fwd(has_list=False) == (BLOCK, 4, 16, 6, 2, 1, WAVE_LONG, 9152)
    assert fwd(has_z=False, ldz=0, ldsave=0, drop_on=True) == BASE                      # neither Z, saved args nor dropout move it
    assert fwd(aggr=(SUM, MEAN, MAX)) == (BLOCK, 4, 16, 7, 2, 1, LIST, 10176)           # planes 3: 6592 + 16 * 16 * 14
    assert bwd(aggr=(SUM, MAX)) == (BLOCK, 4, 16, 7, 2, 1, LIST, 10176)                 # backward: the instantiation's 3 planes
    assert bwd(aggr=(MAX,), ldgu=0) == BASE                                             # one aggregator, the {min, max} instantiation


def test_short_segment_gate_and_empty_calls():
    assert fwd(N=1000, E=16000) == BASE
    assert fwd(N=1000, E=16001) == (NONE, 4, 0, 0, 2, 1, WAVE, 0)
    assert bwd(N=1000, E=16000) == BASE
    assert bwd(N=1000, E=16001) == (NONE, 4, 0, 0, 2, 1, WAVE, 0)
    assert fwd(N=1000, E=16001, has_list=False) == (NONE, 4, 0, 0, 2, 1, WAVE, 0)       # the list plays no part without a first pass
    assert fwd(N=1, E=16) == BASE and fwd(N=1, E=17) == (NONE, 4, 0, 0, 2, 1, WAVE, 0)
    assert fwd(E=0) == (NONE, 4, 0, 0, 2, 1, WAVE, 0)                                   # E == 0: the wave pass writes the empty results
    assert given(E=0) == (NONE, 4, 0, 0, 2, 1, WAVE, 0)
    assert bwd(E=0) == (0,) * 8 and fwd(N=0, E=0) == (0,) * 8 and bwd(N=0, E=5) == (0,) * 8       # nothing launches


def test_vec4_gates():
    assert fwd(T=3, F=5) == (FLAT, 1, 16, 0, 4, 1, LIST, 0)                             # F % 4: 15 columns -> 16 lanes
    for F in (1, 2, 3):                                                                 # F < 4 is never VEC 4, so never block
        assert fwd(T=16 // F + 1, F=F)[:4] == (FLAT, 1, 16, 0)
    assert fwd(T=8, F=2) == FLAT1
    assert fwd(lduv=33) == FLAT1 and fwd(lduv=34) == FLAT1 and fwd(lduv=36) == BASE     # a pitch that is no multiple of 4
    assert fwd(ldz=18) == FLAT1 and fwd(ldz=20) == BASE
    assert fwd(ldz=18, has_z=False) == BASE                                             # ... of an operand the call does not have
    assert fwd(ldsave=18) == FLAT1 and fwd(ldsave=20) == BASE
    assert given(ldi=18) == FLAT1 and given(ldi=20) == BASE
    assert fwd(aligned=False) == FLAT1 and given(aligned=False) == FLAT1 and bwd(aligned=False) == FLAT1
    # the backward's own conditions: gmsg's pitch, and gU's when there is a gU
    assert bwd(ldg=18) == FLAT1 and bwd(ldg=20) == BASE
    assert bwd(ldgu=34) == FLAT1 and bwd(ldgu=36) == BASE and bwd(ldgu=0) == BASE
    assert fwd(N=10, E=161, lduv=33) == (NONE, 1, 0, 0, 4, 1, WAVE, 0)                  # VEC 1 and long segments: the wave kernel alone


def test_pitches_below_the_row():
    """gr_vec4 also asks for pitches >= D.  The forward refuses such calls first (as the query does), so there the clause never
    decides; the backward checks ldg, ldgu and the ldsave it needs, and takes smaller lduv / ldz / unused ldsave at VEC 1."""
    refused("row pitch too small", lduv=15)
    refused("row pitch too small", ldz=12)
    refused("row pitch too small", given=True, lduv=0, ldz=0, has_z=False, ldi=12)
    refused("ldsave=12 < T*F", ldsave=12)
    refused("NULL argument or pitch too small", backward=True, ldg=12, ldgu=32)
    refused("ldgu=12 < T*F", backward=True, ldg=16, ldgu=12)
    refused("ldsave=12 < T*F", backward=True, ldg=16, ldsave=12)
    assert bwd(lduv=12) == FLAT1 and bwd(ldz=12) == FLAT1
    assert bwd(aggr=(SUM, MEAN), ldsave=12, has_stats=True) == FLAT1                    # saved state the list does not need
    assert bwd(aggr=(SUM, MEAN), ldsave=0) == (BLOCK, 4, 16, 7, 2, 1, LIST, 10176)


def test_var_std_and_saved_statistics_leave_the_block_path():
    assert fwd(aggr=(SUM, VAR)) == FLAT4 and fwd(aggr=(STD,)) == FLAT4
    assert fwd(has_stats=True) == FLAT4                                                 # mean / var arrays passed: no block
    assert bwd(has_stats=True) == FLAT4
    assert bwd(aggr=(MEAN, STD), has_stats=True) == FLAT4 and bwd(aggr=(VAR,), has_stats=True) == FLAT4


def test_backward_takes_eight_gradient_blocks():
    assert bwd(aggr=(MIN, MAX), S=4) == BASE                                            # K * S = 8
    assert bwd(aggr=(SUM, MEAN, MIN, MAX), S=2) == (BLOCK, 4, 16, 7, 2, 1, LIST, 10176)
    assert bwd(aggr=(SUM, MEAN, MAX), S=3) == FLAT4                                     # K * S = 9
    assert fwd(aggr=(SUM, MEAN, MAX), S=3) == (BLOCK, 4, 16, 7, 2, 1, LIST, 10176)      # ... which the forward takes
    assert bwd(aggr=(MIN, MAX), S=5) == FLAT4


def test_width_limits():
    # VEC 4: 4095 quads is the flat kernel's last width (the block gate D <= 16380 ends at the same D, long after its LDS budget did)
    assert fwd(T=1, F=16380) == (FLAT, 4, 16, 0, 6, 64, LIST, 0)
    assert fwd(T=1, F=16384) == (NONE, 4, 0, 0, 6, 64, WAVE, 0)
    assert fwd(T=4095, F=4) == (FLAT, 4, 16, 0, 6, 64, LIST, 0)
    assert fwd(T=4096, F=4) == (NONE, 4, 0, 0, 6, 64, WAVE, 0)
    # VEC 1: 4095 columns
    assert fwd(T=1, F=4095) == (FLAT, 1, 16, 0, 6, 64, LIST, 0)
    assert fwd(T=1, F=4096, aligned=False) == (NONE, 1, 0, 0, 6, 64, WAVE, 0)
    assert fwd(T=1, F=4097) == (NONE, 1, 0, 0, 4, 257, WAVE, 0)                         # 4097 = 256 * 16 + 1: 16 lanes waste the fewest
    assert bwd(T=1, F=16380) == (FLAT, 4, 16, 0, 6, 64, LIST, 0) and bwd(T=1, F=16384) == (NONE, 4, 0, 0, 6, 64, WAVE, 0)


# (planes, D) -> nb and lds_bytes = 6592 + nb * D * (4 * planes + 2); None: the flat kernel.  Each pair of rows is the last width of
# an nb step and the first width (a multiple of 4) past it.
LADDER = {
    2: [(212, 16, 40512), (216, 8, 23872), (428, 8, 40832), (432, 4, 23872), (856, 4, 40832), (860, 2, 23792), (1716, 2, 40912),
        (1720, None, 0)],
    3: [(152, 16, 40640), (156, 8, 24064), (304, 8, 40640), (308, 4, 23840), (612, 4, 40864), (616, 2, 23840), (1224, 2, 40864),
        (1228, None, 0)],
    4: [(116, 16, 40000), (120, 8, 23872), (236, 8, 40576), (240, 4, 23872), (476, 4, 40864), (480, 2, 23872), (952, 2, 40864),
        (956, None, 0)],
}
FWD_LIST = {2: (MIN, MAX), 3: (SUM, MEAN, MAX), 4: (SUM, MEAN, MIN, MAX)}               # forward: planes = K
BWD_LIST = {2: (MIN, MAX), 3: (SUM, MEAN, MIN, MAX)}                                    # backward: planes of the instantiation


def ladder_fields(plan):
    return (plan[0], plan[2], plan[3], plan[7])


@pytest.mark.parametrize("planes", [2, 3, 4])
def test_nb_ladder_forward(planes):
    aggr = FWD_LIST[planes]
    needs = 6 if planes == 2 else 7
    for D, nb, lds in LADDER[planes]:
        want = (BLOCK, nb, needs, lds) if nb else (FLAT, 16, 0, 0)
        assert ladder_fields(fwd(T=D // 4, F=4, aggr=aggr, S=2)) == want, (planes, D, "F = 4")
        assert ladder_fields(fwd(T=1, F=D, aggr=aggr, S=2)) == want, (planes, D, "one tower")


@pytest.mark.parametrize("planes", [2, 3])
def test_nb_ladder_backward(planes):
    aggr = BWD_LIST[planes]
    needs = 6 if planes == 2 else 7
    S = 8 // len(aggr)
    for D, nb, lds in LADDER[planes]:
        want = (BLOCK, nb, needs, lds) if nb else (FLAT, 16, 0, 0)
        assert ladder_fields(bwd(T=D // 4, F=4, aggr=aggr, S=S)) == want, (planes, D, "F = 4")
        assert ladder_fields(bwd(T=1, F=D, aggr=aggr, S=S)) == want, (planes, D, "one tower")


def test_forward_and_backward_can_take_different_forms():
    """Four forward planes do not fit at D = 1224, the backward's three do (K3 flat, K4 block); K * S = 9 is the opposite hand-off."""
    aggr = (SUM, MEAN, MIN, MAX)
    assert ladder_fields(fwd(T=1, F=1224, aggr=aggr, S=2)) == (FLAT, 16, 0, 0)
    assert ladder_fields(bwd(T=1, F=1224, aggr=aggr, S=2)) == (BLOCK, 2, 7, 40864)
    assert ladder_fields(fwd(T=1, F=612, aggr=(SUM, MEAN, MAX), S=3)) == (BLOCK, 4, 7, 40864)
    assert ladder_fields(bwd(T=1, F=612, aggr=(SUM, MEAN, MAX), S=3)) == (FLAT, 16, 0, 0)


@pytest.mark.parametrize("per_row,lpr_log,chunks", [(1, 0, 1), (3, 2, 1), (16, 4, 1), (17, 5, 1), (64, 6, 1), (65, 4, 5), (95, 5, 3)])
def test_lane_geometry(per_row, lpr_log, chunks):
    """gr_grid: lanes per row (2^lpr_log) and column chunks.  17 -> 32 lanes (15 idle), 65 -> 16 lanes x 5, 95 -> 32 x 3."""
    assert fwd(T=1, F=4 * per_row, N=6, E=100) == (NONE, 4, 0, 0, lpr_log, chunks, WAVE, 0)
    assert fwd(T=1, F=per_row, N=6, E=100, aligned=False) == (NONE, 1, 0, 0, lpr_log, chunks, WAVE, 0)
    if per_row % 4:
        assert fwd(T=1, F=per_row, N=6, E=100) == (NONE, 1, 0, 0, lpr_log, chunks, WAVE, 0)
    assert fwd(T=1, F=4 * per_row)[4:6] == (lpr_log, chunks) and bwd(T=1, F=4 * per_row)[4:6] == (lpr_log, chunks)


def test_nb_cap_from_the_environment(monkeypatch):
    """MMA_GR_NB (read per call) is where the ladder starts; it never raises nb and values outside 2..16 are ignored."""
    for cap, nb, lds in ((16, 16, 9152), (8, 8, 7872), (4, 4, 7232), (2, 2, 6912)):
        monkeypatch.setenv("MMA_GR_NB", str(cap))
        assert fwd() == (BLOCK, 4, nb, 6, 2, 1, LIST, lds) and bwd() == (BLOCK, 4, nb, 6, 2, 1, LIST, lds)
    monkeypatch.setenv("MMA_GR_NB", "4")
    assert ladder_fields(fwd(T=1, F=860, S=2)) == (BLOCK, 2, 6, 23792)                  # the LDS budget still decides below the cap
    assert ladder_fields(fwd(T=1, F=212, S=2)) == (BLOCK, 4, 6, 15072)                  # 6592 + 4 * 212 * 10
    assert fwd(aggr=(SUM, VAR)) == FLAT4                                                # the flat kernel's 16 nodes are not capped
    for ignored in ("1", "17", "0", "many"):
        monkeypatch.setenv("MMA_GR_NB", ignored)
        assert fwd() == BASE


def refused(message, **kw):
    a = dict(N=N0, E=E0, T=2, F=8, aggr=(MIN, MAX), scalers=(0,), lduv=32, ldz=16, ldsave=16, has_z=True)
    a.update(kw)
    with pytest.raises(_lib.MMALibraryError) as e:
        Fn.gr_plan(**a)
    assert message in str(e.value), str(e.value)


def test_wrong_arguments_are_refused_with_a_message():
    # the checks the query shares with the entry points (gr_open), in their order
    refused("N=-1 E=3000 T=2 F=8 unsupported", N=-1, aggr=None, scalers=None)
    refused("N=1000 E=2147483648 T=2 F=8 unsupported", E=1 << 31)
    refused("N=1000 E=3000 T=4096 F=4096 unsupported", T=4096, F=4096)
    refused("K=0 (1..8) / S=1 (1..8) unsupported", aggr=())
    refused("K=2 (1..8) / S=9 (1..8) unsupported", scalers=(0,) * 9)
    refused("aggregator code 6 unknown", aggr=(MAX, 6))
    refused("scaler code 5 unknown", scalers=(5,))
    # its own
    refused("negative row pitch", ldz=-4)
    refused("give either `inputs` (ldi) or U and V (lduv, ldz)", given=True, ldi=16)
    refused("give either `inputs` (ldi) or U and V (lduv, ldz)", ldi=16)
    refused("saved statistics without ldsave", has_stats=True, ldsave=0)
    refused("ldg / ldgu belong to the backward", ldg=16)
    refused("saved forward state missing", backward=True, ldg=16, ldsave=0)
    refused("saved forward state missing", backward=True, ldg=16, aggr=(SUM, STD))
    Fn.gr_plan(N0, E0, 2, 8, (SUM, MEAN), (0,), backward=True, lduv=32, ldg=16)        # no saved state needed: planned
    L = _lib.lib()
    import ctypes
    codes = (ctypes.c_uint8 * 2)(MIN, MAX)
    assert L.mma_gr_plan(N0, E0, 2, 8, codes, 2, codes, 1, 0, 32, 16, 0, 16, 0, 0, 1, 0, 0, 1, 0, 1, None) != 0
    assert "NULL plan" in L.mma_last_error().decode()
