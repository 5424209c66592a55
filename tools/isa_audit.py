#!/usr/bin/env python3
"""ISA audit of the HIP kernels (no GPU needed: hipcc -S cross-compiles): the two patterns that cost time without showing in the source.

  1. FLAT memory operations.  `cond ? lds_ptr[i] : global_ptr[j]` compiles into ONE flat load from a selected address; a flat load counts in
     vmcnt AND lgkmcnt, so the wait for it is `s_waitcnt vmcnt(0) lgkmcnt(0)` - inside a loop that also stores, a wait for the
     acknowledgement of every store issued before it (round 5: K4's per-edge loop, 0.39 -> 0.34 ms once the loop was split on the condition).
  2. Innermost loops that store AND wait for vmcnt(0): gfx950 has one in-order counter for loads and stores, so a load issued behind
     stores is a load that waits for them (K16's forward epilogue read its bias per stored element: 0.074 -> 0.063 ms with the bias in
     registers before the first store).

    python tools/isa_audit.py [file.hip ...]        (default: every mma_amd/csrc/*.hip; ~3 min for all of them on 8 cores)
    python tools/isa_audit.py --filter 'gr_bwd_block|segsum' mma_amd/csrc/gr_fused.hip mma_amd/csrc/spmm_rows.hip

Exit code 1 when a kernel has flat operations that are not on the allow list below (kernels that take pointer tables by design).

  3. --diff OLD.hip NEW.hip: the check of a refactor that must not move an instruction.  Both files are compiled (OLD may live anywhere:
     its includes resolve next to NEW), kernels are paired by name AS PRINTED (demangled when a demangler is found, else mangled; --rename
     'OLD=NEW' pairs the one old kernel whose name contains OLD with the one new kernel whose name contains NEW), comments, labels and directives are dropped, and every kernel is reported as
       identical   the same instruction text (tier A);
       tier B      same registers / scratch / LDS / occupancy, the same opcode sequence inside every innermost loop and the same number
                   of MFMA, LDS, vector-memory, s_waitcnt and s_barrier instructions - with a unified diff and both resource lines.
                   Tier B says nothing about results (a changed constant is tier B): READ the printed diff;
       DIFFERENT   anything else (exit code 1, as for a kernel without a partner).

    python tools/isa_audit.py --diff old/gemm_x3.hip mma_amd/csrc/gemm_x3.hip --rename 'k256p_kernel(=k256_kernel<true' \\
                              --rename 'colgroup_k256_kernel(=k256_kernel<false'"""
import argparse
import concurrent.futures
import difflib
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = "-O3 -std=c++17 -fPIC -ffp-contract=off --offload-arch=gfx950 -fno-gpu-rdc -Wno-unused-function -S --cuda-device-only".split()
# flat operations by design: Adam walks a table of tensor pointers; the halo pack kernels select between two row sources per block;
# the block backward of GR keeps ONE flat load in its generic (un-staged or by-edge-id) form of the edge loop
ALLOW = re.compile(r"adam_kernel|pack_blocks_kernel|gr_bwd_block_kernel")


def asm_of(src, include_dir=None, tag=""):
    out = os.path.join(tempfile.gettempdir(), "isa_audit_" + tag + os.path.basename(src) + ".s")
    inc = ["-I" + include_dir] if include_dir else []
    subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + inc + [src, "-o", out], check=True, cwd=os.path.dirname(src), stderr=subprocess.DEVNULL)
    return src, open(out).read()


def kernel_parts(asm):
    """(mangled name, everything from the kernel's label to the next kernel's: code, then the resource comments)"""
    for part in re.split(r"\n(?=_Z[\w]+:\s*(?:;.*)?\n)", asm):
        m = re.match(r"(_Z\w+):", part)
        if m:
            yield m.group(1), part


def kernels(asm):
    for name, part in kernel_parts(asm):
        yield name, part.split(".Lfunc_end")[0].split("\n")


def innermost_loops(lines):
    labels, loops = {}, []
    for n, line in enumerate(lines):
        m = re.match(r"(\.LBB\w+):", line.strip())
        if m:
            labels[m.group(1)] = n
    for n, line in enumerate(lines):
        t = line.strip()
        if t.startswith(("s_cbranch", "s_branch")):
            tgt = t.split()[-1]
            if tgt in labels and labels[tgt] < n:
                loops.append((labels[tgt], n))
    return [(a, b) for (a, b) in loops if not any(a <= c and d <= b and (c, d) != (a, b) for (c, d) in loops)]


def demangle(names):
    """mangled -> demangled, by the first demangler found (ROCm's llvm-cxxfilt, else one on PATH); without one the names stay mangled"""
    for tool in ("/opt/rocm/lib/llvm/bin/llvm-cxxfilt", "/opt/rocm/llvm/bin/llvm-cxxfilt", shutil.which("llvm-cxxfilt"), shutil.which("c++filt")):
        try:
            out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout
            return dict(zip(names, out.split("\n")))
        except Exception:
            continue
    return {n: n for n in names}


RESOURCES = ("NumVgprs", "NumAgprs", "TotalNumSgprs", "ScratchSize", "LDSByteSize", "Occupancy")
CLASSES = (r"v_mfma", r"ds_", r"(buffer|global)_load", r"(buffer|global)_(store|atomic)", r"s_waitcnt", r"s_barrier")


def resources(part):
    """the register / scratch / LDS / occupancy figures hipcc prints as comments behind a kernel's code"""
    found = {k: v for k, v in re.findall(r";\s*(\w+):\s*(\d+)", part.split(".Lfunc_end", 1)[-1])}
    return " ".join("%s=%s" % (k, found.get(k, "?")) for k in RESOURCES)


def instructions(lines):
    """instruction text only: no comments, labels or directives; block labels lose the kernel's index (it moves with the kernel order)"""
    out = []
    for line in lines[1:]:
        t = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0].strip())
        if t and not t.startswith(".") and not t.endswith(":"):
            out.append(re.sub(r"\s+", " ", t))
    return out


def loop_opcodes(lines):
    body = [line.split(";")[0].strip() for line in lines]
    return [[x.split()[0] for x in body[a:b + 1] if x and not x.startswith(".") and not x.endswith(":")] for a, b in innermost_loops(lines)]


def tier_b(old, new, old_ins, new_ins, old_res, new_res):
    count = lambda ins: [sum(1 for x in ins if re.match(c, x)) for c in CLASSES]
    return old_res == new_res and "ScratchSize=0" in new_res and loop_opcodes(old) == loop_opcodes(new) and count(old_ins) == count(new_ins)


def diff_main(old_src, new_src, renames, name_filter):
    old_src, new_src = os.path.abspath(old_src), os.path.abspath(new_src)
    with concurrent.futures.ThreadPoolExecutor(max_workers=2) as ex:
        fo = ex.submit(asm_of, old_src, os.path.dirname(new_src), "old_")
        fn = ex.submit(asm_of, new_src, None, "new_")
        sides = []
        for asm in (fo.result()[1], fn.result()[1]):
            parts = dict(kernel_parts(asm))
            names = demangle(list(parts))
            sides.append({names[k]: part for k, part in parts.items()})
    old, new = sides
    for a, b in renames:
        was, now = [n for n in old if a in n], [n for n in new if b in n]
        if len(was) != 1 or len(now) != 1:
            sys.exit("--rename %s=%s: matches %d old and %d new kernel names, need exactly one of each" % (a, b, len(was), len(now)))
        old[now[0]] = old.pop(was[0])
    tally = {"identical": [], "tier B": [], "DIFFERENT": [], "unpaired": sorted(set(old) ^ set(new))}
    for name in sorted(set(old) & set(new)):
        if name_filter and not re.search(name_filter, name):
            continue
        ol, nl = old[name].split(".Lfunc_end")[0].split("\n"), new[name].split(".Lfunc_end")[0].split("\n")
        oi, ni = instructions(ol), instructions(nl)
        if oi == ni:
            tally["identical"].append(name)
            continue
        ores, nres = resources(old[name]), resources(new[name])
        verdict = "tier B" if tier_b(ol, nl, oi, ni, ores, nres) else "DIFFERENT"
        tally[verdict].append(name)
        print("%s: %s (%d -> %d instructions)\n  old: %s\n  new: %s" % (verdict, name, len(oi), len(ni), ores, nres))
        print("\n".join(difflib.unified_diff(oi, ni, "old", "new", n=2, lineterm="")))
    for name in tally["unpaired"]:
        print("unpaired: %s (%s only)" % (name, "old" if name in old else "new"))
    print("%d kernels: %d identical, %d tier B, %d different, %d unpaired" % (
        sum(len(v) for v in tally.values()), len(tally["identical"]), len(tally["tier B"]), len(tally["DIFFERENT"]), len(tally["unpaired"])))
    for name in tally["tier B"]:
        print("  tier B: " + name)
    return 1 if tally["DIFFERENT"] or tally["unpaired"] else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("files", nargs="*")
    ap.add_argument("--diff", nargs=2, metavar=("OLD.hip", "NEW.hip"), help="compare the two files' device code kernel by kernel")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW", help="with --diff: pair the old kernel whose printed name contains OLD with the new one whose name contains NEW")
    ap.add_argument("--filter", default="", help="regular expression on the demangled kernel name")
    ap.add_argument("--loops", action="store_true", help="also list innermost loops that store and wait for vmcnt(0)")
    args = ap.parse_args()
    if args.diff:
        return diff_main(args.diff[0], args.diff[1], [r.split("=", 1) for r in args.rename], args.filter)
    files = [os.path.abspath(f) for f in args.files] or sorted(glob.glob(os.path.join(ROOT, "mma_amd", "csrc", "*.hip")))
    bad = 0
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, len(files))) as ex:
        for src, asm in ex.map(asm_of, files):
            ks = list(kernels(asm))
            names = demangle([k for k, _ in ks])
            n_flat = n_k = 0
            for k, lines in ks:
                name = names[k]
                if args.filter and not re.search(args.filter, name):
                    continue
                n_k += 1
                body = [line.strip() for line in lines]
                flat = [line for line in body if re.match(r"flat_(load|store|atomic)", line)]
                if flat:
                    n_flat += 1
                    ok = bool(ALLOW.search(name))
                    bad += 0 if ok else 1
                    print("%s  %s: %d flat operation(s)%s" % (os.path.basename(src), name[:110], len(flat), " (allowed)" if ok else "  <-- check"))
                if args.loops:
                    for a, b in innermost_loops(lines):
                        lb = [x for x in body[a:b + 1] if x and not x.startswith(";")]
                        st = sum(1 for x in lb if re.match(r"(global|buffer|flat)_(store|atomic)", x))
                        w0 = sum(1 for x in lb if x.startswith("s_waitcnt") and "vmcnt(0)" in x)
                        if st and w0 and len(lb) < 400:
                            print("%s  %s: loop of %d instructions with %d store(s) and %d vmcnt(0) wait(s)" % (
                                os.path.basename(src), name[:90], len(lb), st, w0))
            print("%s: %d kernels, %d with flat operations" % (os.path.basename(src), n_k, n_flat))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
