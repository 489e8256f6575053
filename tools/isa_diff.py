r"""Dev tool: codegen gate between two builds of one translation unit.  Inputs per side: the device assembly
(hipcc <product flags> --cuda-device-only -S) and the remarks of -Rpass-analysis=kernel-resource-usage (stderr of that
compile).  Prints the resource table (parent | branch per kernel) or the per-kernel diff of the instruction streams with
comments, .loc / .file / .cfi lines, labels' debug suffixes, local labels' function ordinals and metadata stripped.
usage: python tools/isa_diff.py resources parent.remarks branch.remarks [tu]
       python tools/isa_diff.py isa parent.s branch.s [tu]
       python tools/isa_diff.py functions parent.s branch.s [tu] [--rename REGEX REPLACEMENT]...
functions: like isa, but over EVERY function of the unit - kernels and the device functions that stayed out of line - paired
by MANGLED name, each --rename applied (re.sub) to the names and to the instruction lines of both sides first: for a helper
that gained a defaulted template argument, e.g. --rename '(sort_keys_descILi\d+E)Li0E' '\1'.  One summary line per unit.
tu: the translation unit's name for the headings (default: the branch file's name up to its first dot + ".hip")
--same NAME (repeatable, after the other arguments): a template argument that the branch added with a default, e.g.
ListNoElig - kernels are paired by demangled name with ", NAME" / "<NAME>" removed, so f<S, NAME> (or f<NAME>) of the branch
is judged against the parent's f<S> (or f).
--same-branch NAME: the same, applied to the branch's names alone - for an added trailing argument whose default (false, 0)
also occurs among the parent's own arguments, where --same would rename the parent's kernels too."""
import difflib
import os
import re
import subprocess
import sys


SAME = []           # --same: template arguments dropped from the demangled names
SAME_BRANCH = []    # --same-branch: a trailing template argument dropped from the branch's demangled names only


def demangle(names, branch=False):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    res = {}
    for n, d in zip(names, out):
        d = re.sub(r"\(.*", "", d).replace("amdrec::", "")
        for t in SAME_BRANCH if branch else []:
            d = d[:-len(", " + t + ">")] + ">" if d.endswith(", " + t + ">") else d
        for t in SAME:
            d = d.replace(", " + t + ">", ">").replace(", " + t + " >", " >").replace("<" + t + ">", "")
            d = d.replace(", " + t + ", ", ", ")             # ... or in front of a trailing pack: f<S, A, NAME, P...> is f<S, A, P...>
        if SAME:
            d = d.replace("<>", "")                          # a kernel that gained an (empty) trailing pack: f<> is f
        res[n] = re.sub(r"^void (\w+)$", r"\1", d.replace("> >", ">>"))
    return res


def by_name(table, branch=False):
    """mangled name -> value  =>  demangled (and --same-normalised) name -> value"""
    names = demangle(sorted(table), branch)
    return {names[n]: v for n, v in table.items()}


def resources(path):
    res, cur = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = res.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1)] = m.group(2)
    return res


def kernels(path, everything=False):
    """kernel name -> its instruction lines (between the kernel's label and its s_endpgm / .Lfunc_end).  Local labels
    (.LBB<n>_<m>, .LJTI<n>_<m>, .LCPI<n>_<m>) lose <n>, the function's ordinal in the translation unit: a kernel that joins or
    leaves the unit renumbers every later function without moving an instruction."""
    out, cur = {}, None
    for line in open(path):
        line = re.sub(r"(\.L[A-Za-z]+)\d+_(\d+)", r"\1_\2", line.split(";")[0].rstrip())
        s = line.strip()
        m = re.match(r"^(\w+):$", s)
        if m and cur is None and not s.startswith(".L"):
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        if s.startswith(".Lfunc_end"):
            cur = None
            continue
        if not s or s.startswith((".loc", ".file", ".cfi", ".p2align", ".section", ".amdhsa", ".end_amdhsa", ".Ltmp", ".type", ".size", ".text")):
            continue
        cur.append(s)
    return out if everything else {k: v for k, v in out.items() if any(i.startswith("s_endpgm") for i in v)}


def main():
    argv = sys.argv[1:]
    while "--same" in argv:
        i = argv.index("--same")
        SAME.append(argv[i + 1])
        del argv[i:i + 2]
    while "--same-branch" in argv:
        i = argv.index("--same-branch")
        SAME_BRANCH.append(argv[i + 1])
        del argv[i:i + 2]
    renames = []
    while "--rename" in argv:
        i = argv.index("--rename")
        renames.append((re.compile(argv[i + 1]), argv[i + 2]))
        del argv[i:i + 3]
    mode, a, b = argv[:3]
    tu = argv[3] if len(argv) > 3 else os.path.basename(b).split(".")[0] + ".hip"
    if mode == "functions":
        def renamed(text):
            for pat, rep in renames:
                text = pat.sub(rep, text)
            return text
        fa, fb = ({renamed(k): [renamed(i) for i in v] for k, v in kernels(f, True).items() if not k.startswith("__hip_cuid_")}
                  for f in (a, b))
        both = sorted(set(fa) & set(fb))
        differ = [k for k in both if fa[k] != fb[k]]
        print(f"{tu}: {len(both)} functions and kernels in both, {len(both) - len(differ)} identical, different: {differ}; only in "
              f"the parent: {sorted(set(fa) - set(fb))}; only in the branch: {sorted(set(fb) - set(fa))}")
        return 1 if differ else 0
    if mode == "resources":
        ra, rb = by_name(resources(a)), by_name(resources(b), True)
        names = {n: n for n in set(ra) | set(rb)}
        cols = [("VGPR", "VGPRs"), ("AGPR", "AGPRs"), ("SGPR", "TotalSGPRs"), ("scratch", "ScratchSize [bytes/lane]"),
                ("spilled VGPRs", "VGPRs Spill"), ("LDS", "LDS Size [bytes/block]"), ("occ", "Occupancy [waves/SIMD]")]
        print(f"Kernel resource usage of {tu} (product flags + -Rpass-analysis=kernel-resource-usage), parent | branch")
        print("conditions per kernel: VGPR, AGPR, scratch, spilled VGPRs, LDS and occupancy equal (SGPR shown for information)\n")
        print("".join(f"{c[0]:>15}" for c in cols) + "  ok  kernel")
        bad = 0
        for n in sorted(names, key=names.get):
            pa, pb = ra.get(n, {}), rb.get(n, {})
            ok = all(pa.get(k) == pb.get(k) for _, k in cols if k != "TotalSGPRs")
            both = bool(pa) and bool(pb)                        # a kernel of one side only is listed, not judged
            bad += both and not ok
            mark = ("yes" if ok else "NO ") if both else ("old" if pa else "new")
            print("".join(f"{pa.get(k, '-') + '|' + pb.get(k, '-'):>15}" for _, k in cols) + f"  {mark} {names[n]}")
        print(f"\n{len(set(ra) & set(rb))} kernels in both, {bad} outside the conditions; {len(set(ra) - set(rb))} only in the "
              f"parent (old), {len(set(rb) - set(ra))} only in the branch (new)")
        return 1 if bad else 0
    ka, kb = by_name(kernels(a)), by_name(kernels(b), True)
    names = {n: n for n in set(ka) | set(kb)}
    differ = 0
    print(f"Instruction streams of {tu}'s kernels, parent against branch (comments, .loc / .file lines and metadata stripped)\n")
    for n in sorted(names, key=names.get):
        if n not in ka or n not in kb:                     # left or joined the unit: listed, not compared
            print(f"{names[n]}: ONLY IN {'PARENT' if n in ka else 'BRANCH'}")
            continue
        ia, ib = ka[n], kb[n]
        cnt = lambda v: (sum(1 for i in v if not i.endswith(":") and not i.startswith(".")), sum(1 for i in v if i.startswith("v_mfma")))
        same = ia == ib
        differ += not same
        print(f"{names[n]}: {'IDENTICAL' if same else 'DIFFERENT'}  instructions {cnt(ia)[0]} | {cnt(ib)[0]}  MFMAs {cnt(ia)[1]} | {cnt(ib)[1]}")
        if not same:
            d = list(difflib.unified_diff(ia, ib, "parent", "branch", n=1, lineterm=""))
            print(f"  {sum(1 for l in d if l[:1] in '+-' and l[:3] not in ('+++', '---'))} changed lines; first hunks:")
            print("\n".join("  " + l for l in d[:60]))
    print(f"\n{len(set(ka) & set(kb))} kernels in both, {differ} with a different instruction stream; "
          f"{len(set(ka) - set(kb))} only in the parent, {len(set(kb) - set(ka))} only in the branch")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
