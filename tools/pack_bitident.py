"""Dev tool: do two versions of the host-side ranker packing (amdrec/weights.py pack_ranker) produce the same bytes?  Per case it
takes from pack_ranker(...) on device "cpu": the task list, every scalar field of RankerParams (layers[] and x3 included) and,
for every non-null pointer field, the dtype, shape and SHA-256 of the tensor in pk._keep with that data_ptr().
  architectures  "demo" and every entry of tests/cases.py RANKER_SURFACE
  knobs          fuse_attention x x6 x (x3 off | x3 on: x3_variant 16 / 32, fold_first_attention off / on / on with
                 cache_first_ffn, x3_min_rows 1 / 0, x3_cs_max_rows 0 / -1): 100 packings per architecture
Each argument is a directory that holds an ``amdrec`` package (for the parent commit: a ``git worktree`` of it); each package
runs in its own child process and never touches a GPU.  The parent process compares the two sides field by field, prints the
differing field paths and exits non-zero on any difference.  Compare within one run on one machine: float64 BLAS results may
differ in the last bit between machines, so no digest is a golden value.  Log: profiles/pack_once_bitident.log.
usage: python tools/pack_bitident.py DIR_A DIR_B"""
import ctypes as C
import hashlib
import itertools
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CHILD_SECONDS = 600


def knob_sets():
    x3_sets = [dict(x3=False)] + [
        dict(x3=True, x3_variant=v, fold_first_attention=fold, cache_first_ffn=cache, x3_min_rows=mr, x3_cs_max_rows=cs)
        for v, (fold, cache), mr, cs in itertools.product((16, 32), ((False, False), (True, False), (True, True)), (1, 0), (0, -1))]
    return [dict(fuse_attention=fuse, x6=x6, **x3) for fuse, x6, x3 in itertools.product((True, False), (True, False), x3_sets)]


def describe(obj, ctype, path, tensors, out):
    if issubclass(ctype, C.Structure):
        for name, ftype in ctype._fields_:
            describe(getattr(obj, name), ftype, f"{path}.{name}", tensors, out)
    elif issubclass(ctype, C.Array):
        for i in range(ctype._length_):
            describe(obj[i], ctype._type_, f"{path}[{i}]", tensors, out)
    elif ctype is C.c_void_p:
        if obj:
            t = tensors.get(obj)
            out[path] = "NOT IN pk._keep" if t is None else [
                str(t.dtype), list(t.shape), hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()]
        else:
            out[path] = None
    else:
        out[path] = obj


def child(pkg_dir, out_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, pkg_dir)
    from amdrec import weights
    from tests import cases
    assert os.path.samefile(os.path.dirname(os.path.dirname(weights.__file__)), pkg_dir), weights.__file__
    result = {}
    for arch in ["demo"] + list(cases.RANKER_SURFACE):
        user, ad, nnum, sd = cases.ranker_case("demo", "scaled")[:4] if arch == "demo" else cases.surface_ranker_case(arch)
        for kw in knob_sets():
            p, pk, tasks = weights.pack_ranker(sd, list(user), list(ad), nnum, "cpu", **kw)
            out = {"tasks": list(tasks)}
            describe(p, type(p), "p", {t.data_ptr(): t for t in reversed(pk._keep)}, out)
            result[f"{arch}/" + ",".join(f"{k}={v}" for k, v in kw.items())] = out
    with open(out_path, "w") as f:
        json.dump(result, f)


def main():
    if sys.argv[1] == "--child":
        return child(sys.argv[2], sys.argv[3])
    dirs = [os.path.abspath(d) for d in sys.argv[1:3]]
    sides = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, d in enumerate(dirs):
            path = os.path.join(tmp, f"pack_bitident_{i}.json")
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", d, path], timeout=CHILD_SECONDS)
            if r.returncode != 0:
                print(json.dumps({"dir": d, "exit": r.returncode, "result": "child failed"}))
                return 1
            with open(path) as f:
                sides.append(json.load(f))
    a, b = sides
    differ = [f"{case}: only one side packed it" for case in sorted(set(a) ^ set(b))]
    for case in sorted(set(a) & set(b)):
        differ += [f"{case}: {k}: {a[case].get(k, 'absent')!r} != {b[case].get(k, 'absent')!r}"
                   for k in sorted(set(a[case]) | set(b[case])) if a[case].get(k, "absent") != b[case].get(k, "absent")]
    for arch in sorted({c.split("/")[0] for c in a}):
        mine = [c for c in a if c.startswith(arch + "/")]
        bad = sum(any(d.startswith(c + ":") for d in differ) for c in mine)
        x3 = sum(a[c]["p.x3.stream"] is not None for c in mine)
        hc = sum(a[c]["p.x3.stream_hc"] is not None for c in mine)
        print(f"{'equal ' if not bad else 'DIFFER'} {arch}: {len(mine)} packings ({x3} with the x3 stream, {hc} with the hidden-cache "
              f"stream), {sum(len(a[c]) for c in mine)} fields, {bad} packings differ")
    for d in differ:
        print("    " + d)
    sha = [hashlib.sha256(json.dumps(s, sort_keys=True).encode()).hexdigest() for s in sides]
    print(json.dumps({"dirs": sys.argv[1:3], "packings": len(a), "fields": sum(len(v) for v in a.values()),
                      "differing_fields": len(differ), "sha256": sha, "result": "byte-identical" if not differ else "DIFFERENT"}))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
