#!/usr/bin/env python3
"""k_spmm_seg's instantiations and their resources, from the compiler's remarks.

    hipcc <the Makefile's HIPFLAGS> --cuda-device-only -Rpass-analysis=kernel-resource-usage \\
        -c csrc/lz_spmm.hip -o /dev/null 2> remarks.txt
    scripts/seg_store_resources.py parent_remarks.txt new_remarks.txt

Prints one table per file, keyed by (T, CAP, WIN, MODE, store), and compares them: the same
instantiations; equal LDS and occupancy; no scratch, no spills; VGPRs no higher.  Exit 1 otherwise.
Instantiations of a store in ADDED that only the new file has are a new store's: listed, and held
to no scratch and no spills.
Both spellings of the store are read: the six booleans (YCM, EPI, PF, AX3, DOT, AX4) and the
SegStore enumerator.
"""
import re
import sys

STORES = ["Rows", "ColMajor", "Beta2", "Terms3", "Terms3Dots", "Terms4", "ShiftDots", "Terms4Dots", "RowScale",
          "RowScaleDots"]
ADDED = {"ShiftDots", "Terms4Dots", "RowScale", "RowScaleDots"}  # stores younger than the six: a parent file need not have them
BOOLS = {(0, 0, 0, 0, 0): "Rows", (1, 0, 0, 0, 0): "ColMajor", (0, 1, 0, 0, 0): "Beta2", (0, 0, 1, 0, 0): "Terms3",
         (0, 0, 1, 1, 0): "Terms3Dots", (0, 0, 1, 0, 1): "Terms4"}
HEAD = r"k_spmm_segI([fd])Li\d+ELi\d+ELi(\d+)ELb([01])ELi([01])E"
OLD = re.compile(HEAD + r"Lb([01])ELb([01])ELb([01])ELb([01])ELb([01])ELb([01])EE")
NEW = re.compile(HEAD + r"LNS_8SegStoreE(\d)ELb([01])EE")
FIELDS = {"TotalSGPRs": "sgpr", "VGPRs": "vgpr", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occ",
          "SGPRs Spill": "sspill", "VGPRs Spill": "vspill", "LDS Size [bytes/block]": "lds"}


def key_of(name):
    m = OLD.search(name)
    if m:
        t, cap, win, mode, ycm, epi, pf, ax3, dot, ax4 = m.groups()
        store = BOOLS[tuple(int(v) for v in (ycm, epi, ax3, dot, ax4))]
    else:
        m = NEW.search(name)
        if not m:
            return None
        t, cap, win, mode, st, pf = m.groups()
        store = STORES[int(st)]
    return ("fp64" if t == "d" else "fp32", int(cap), int(win), int(mode), store + ("+PF" if pf == "1" else ""))


def read(path):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+(.*?)\s+\[-Rpass-analysis", line)
        if not m:
            continue
        text = m.group(1)
        if text.startswith("Function Name:"):
            cur = key_of(text)
            if cur is not None:
                assert cur not in out, cur
                out[cur] = {}
        elif cur is not None:
            name, _, val = text.rpartition(": ")
            if name in FIELDS:
                out[cur][FIELDS[name]] = int(val)
    return out


def table(title, res):
    print(f"# {title}: {len(res)} instantiations, {sum(k[0] == 'fp64' for k in res)} fp64, "
          f"{sum(k[0] == 'fp32' for k in res)} fp32")
    print(f"{'T':5} {'CAP':>4} {'WIN':>3} {'MODE':>4} {'store':11} {'VGPR':>4} {'SGPR':>4} {'LDS':>6} {'occ':>3} "
          f"{'scratch':>7} {'spills':>6}")
    for k in sorted(res):
        r = res[k]
        print(f"{k[0]:5} {k[1]:>4} {k[2]:>3} {k[3]:>4} {k[4]:11} {r['vgpr']:>4} {r['sgpr']:>4} {r['lds']:>6} {r['occ']:>3} "
              f"{r['scratch']:>7} {r['sspill'] + r['vspill']:>6}")
    print()


def main():
    old, new = read(sys.argv[1]), read(sys.argv[2])
    table("parent", old)
    table("new", new)
    bad = []
    added = {k for k in set(new) - set(old) if k[4] in ADDED}
    for k in sorted(added):
        n = new.pop(k)
        print(f"# added {k}: VGPR {n['vgpr']}, SGPR {n['sgpr']}, LDS {n['lds']}, occupancy {n['occ']}")
        if n["scratch"] or n["sspill"] or n["vspill"]:
            bad.append(f"{k}: scratch or spills {n}")
    if set(old) != set(new):
        bad.append(f"instantiations differ: only parent {sorted(set(old) - set(new))}, only new {sorted(set(new) - set(old))}")
    for k in sorted(set(old) & set(new)):
        o, n = old[k], new[k]
        if n["lds"] != o["lds"] or n["occ"] != o["occ"] or n["vgpr"] > o["vgpr"] or n["scratch"] or n["sspill"] or n["vspill"]:
            bad.append(f"{k}: parent {o}, new {n}")
        elif n["vgpr"] != o["vgpr"] or n["sgpr"] != o["sgpr"]:
            print(f"# moved {k}: VGPR {o['vgpr']} -> {n['vgpr']}, SGPR {o['sgpr']} -> {n['sgpr']}")
    print("# check: " + ("same instantiations; LDS and occupancy equal; no scratch, no spills; no VGPR count higher"
                         if not bad else "FAILED"))
    for b in bad:
        print("# " + b)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
