"""tools/isa_audit.py's parsing on a synthetic listing (the real audit compiles every kernel: minutes, run by hand - DESIGN.md 7)."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("isa_audit", os.path.join(ROOT, "tools", "isa_audit.py"))
isa_audit = importlib.util.module_from_spec(spec)
spec.loader.exec_module(isa_audit)

ASM = """
\t.text
_ZN3mma5firstEv:                        ; @_ZN3mma5firstEv
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
.LBB0_1:                                ; =>This Loop Header: Depth=1
\tglobal_load_dword v1, v[2:3], off
.LBB0_2:                                ;   Parent Loop BB0_1 Depth=1
\tflat_load_dword v4, v[5:6]
\ts_waitcnt vmcnt(0) lgkmcnt(0)
\tglobal_store_dwordx4 v[7:8], v[9:12], off nt
\ts_cbranch_execnz .LBB0_2
\ts_cbranch_scc1 .LBB0_1
\ts_endpgm
.Lfunc_end0:
_ZN3mma6secondEv:                       ; @_ZN3mma6secondEv
.LBB1_1:
\tds_read_b32 v1, v2
\ts_waitcnt lgkmcnt(0)
\tglobal_store_dword v[3:4], v1, off
\ts_cbranch_execnz .LBB1_1
\ts_endpgm
.Lfunc_end1:
"""


def test_kernels_and_innermost_loops_of_a_listing():
    ks = dict(isa_audit.kernels(ASM))
    assert set(ks) == {"_ZN3mma5firstEv", "_ZN3mma6secondEv"}
    first = ks["_ZN3mma5firstEv"]
    loops = isa_audit.innermost_loops(first)
    assert len(loops) == 1                                    # the outer loop contains the inner one: only the inner is innermost
    a, b = loops[0]
    body = [line.strip() for line in first[a:b + 1]]
    assert any(x.startswith("flat_load") for x in body) and any("vmcnt(0)" in x for x in body) and any(x.startswith("global_store") for x in body)
    second = ks["_ZN3mma6secondEv"]
    (a2, b2), = isa_audit.innermost_loops(second)
    assert not any("vmcnt" in line for line in second[a2:b2 + 1])      # an LDS read ahead of a store waits on lgkmcnt only


def test_the_allow_list_names_the_kernels_that_take_pointer_tables():
    assert isa_audit.ALLOW.search("void mma::adam_kernel<true>(...)") and isa_audit.ALLOW.search("mma::pack_blocks_kernel<false>")
    assert not isa_audit.ALLOW.search("mma::segsum_block_kernel(mma::SegSumParams)")


# ---- --diff: identical / tier B / DIFFERENT on synthetic listings -----------------------------------------------------------------------
def _listing(index, body, vgprs=12, lds=0):
    return ("_ZN3mma4tileEv:                         ; @_ZN3mma4tileEv\n"
            "\ts_load_dwordx2 s[0:1], s[4:5], 0x0    ; kernarg\n" + body +
            "\ts_endpgm\n.Lfunc_end%d:\n\t.size\t_ZN3mma4tileEv, .Lfunc_end%d-_ZN3mma4tileEv\n"
            "; NumVgprs: %d\n; NumAgprs: 0\n; TotalNumSgprs: 20\n; ScratchSize: 0\n; LDSByteSize: %d bytes/workgroup (compile time only)\n"
            "; Occupancy: 8\n" % (index, index, vgprs, lds))


_LOOP = ("\ts_mov_b32 %s, 0x45000000\n"
         ".LBB%d_1:                                ; =>This Inner Loop Header: Depth=1\n"
         "\tds_read_b128 v[0:3], v8\n\ts_waitcnt lgkmcnt(0)\n\tv_mfma_f32_32x32x16_f16 a[0:15], v[0:3], v[4:7], a[0:15]\n"
         "\tbuffer_store_dword v9, v10, s[0:3], %s offen nt\n\ts_cbranch_scc1 .LBB%d_1\n")


def _compare(old, new):
    (_, op), = isa_audit.kernel_parts(old)
    (_, np_), = isa_audit.kernel_parts(new)
    ol, nl = op.split(".Lfunc_end")[0].split("\n"), np_.split(".Lfunc_end")[0].split("\n")
    oi, ni = isa_audit.instructions(ol), isa_audit.instructions(nl)
    return oi == ni, isa_audit.tier_b(ol, nl, oi, ni, isa_audit.resources(op), isa_audit.resources(np_))


def test_diff_ignores_comments_labels_directives_and_the_kernel_index_of_block_labels():
    old = _listing(3, _LOOP % ("s6", 3, "s6", 3))
    new = _listing(7, "\t.p2align 8\n\t; a comment line\n" + _LOOP % ("s6", 7, "s6", 7))
    assert isa_audit.instructions(old.split("\n"))[0].startswith("s_load_dwordx2") and "kernarg" not in isa_audit.instructions(old.split("\n"))[0]
    assert _compare(old, new) == (True, True)
    assert isa_audit.resources(old) == "NumVgprs=12 NumAgprs=0 TotalNumSgprs=20 ScratchSize=0 LDSByteSize=0 Occupancy=8"


def test_diff_tier_b_is_renumbered_scalars_outside_and_the_same_opcodes_inside_the_loops():
    old = _listing(0, _LOOP % ("s6", 0, "s6", 0))
    assert _compare(old, _listing(0, _LOOP % ("s9", 0, "s9", 0))) == (False, True)         # another scalar register: same opcodes, counts, resources
    # a changed constant is tier B as well: the tier says nothing about results, the printed diff has to be read
    assert _compare(old, _listing(0, (_LOOP % ("s6", 0, "s6", 0)).replace("0x45000000", "0x44800000"))) == (False, True)


def test_diff_different_when_resources_loop_opcodes_or_memory_counts_change():
    old = _listing(0, _LOOP % ("s6", 0, "s6", 0))
    assert _compare(old, _listing(0, _LOOP % ("s9", 0, "s9", 0), vgprs=16)) == (False, False)              # more registers
    assert _compare(old, _listing(0, _LOOP % ("s9", 0, "s9", 0), lds=8192)) == (False, False)              # an array promoted to LDS
    extra_in_loop = (_LOOP % ("s6", 0, "s6", 0)).replace("\ts_cbranch_scc1", "\tv_readfirstlane_b32 s2, v0\n\ts_cbranch_scc1")
    assert _compare(old, _listing(0, extra_in_loop)) == (False, False)                                      # another opcode inside the loop
    store_outside = _LOOP % ("s6", 0, "s6", 0) + "\tbuffer_store_dword v9, v10, s[0:3], 0 offen\n"
    assert _compare(old, _listing(0, store_outside)) == (False, False)                                      # one more store in the kernel
