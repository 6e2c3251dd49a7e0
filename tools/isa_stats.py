"""Static instruction mix of the kernels of a csrc/*.hip file (no GPU needed): compiles with -save-temps and histograms the ISA.

    python tools/isa_stats.py color_mfma.hip 'k_color_mfmaILi8ELb1' [--top 30] [-DO2345_TILES_KERNEL]

With --compare DIR the same unit is compiled a second time from DIR (the csrc directory of another tree, e.g. of the parent commit) and every kernel
whose name matches is printed as one line, "DIR -> this tree": registers, LDS, scratch, occupancy, instruction counts, and whether the instructions are
the same once labels are numbered in order of appearance ("identical", or how many lines a line diff leaves over; renamed registers count).  DIR
must lie in its tree (csrc includes ../../include/o2345.h).  The pattern may be omitted:

    python tools/isa_stats.py color_pts.hip --compare ../parent/one-2-3-45_amd/csrc"""
import collections
import difflib
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import importlib
B = importlib.import_module("one-2-3-45_amd.build")

META = ("NumVgprs", "NumAgprs", "TotalNumSgprs", "LDSByteSize", "ScratchSize", "Occupancy", "codeLenInByte")


def kernels(csrc, src, pat, defines):
    """-> {mangled name: (instruction lines, resource dict)} of the kernels of csrc/src whose name contains pat, at build.py's flags + defines"""
    d = tempfile.mkdtemp(prefix="isa_")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + B.FLAGS + B.EXTRA_FLAGS.get(src, []) + defines + ["-save-temps", "-c", os.path.join(csrc, src), "-o", os.path.join(d, "o.o")]
    subprocess.check_call(cmd, cwd=d, stderr=subprocess.DEVNULL)
    sfile = [f for f in os.listdir(d) if f.endswith("gfx950.s")][0]
    s = open(os.path.join(d, sfile)).read().split("\n")
    amdhsa = {l.split()[1] for l in s if l.strip().startswith(".amdhsa_kernel ")}
    out = {}
    for st in [i for i, l in enumerate(s) if re.match(r"^_Z\w*" + re.escape(pat) + r"\w*:", l) and l.split(":")[0] in amdhsa]:
        end = next(i for i in range(st, len(s)) if s[i].startswith(".Lfunc_end"))
        body = [l.split(";")[0].strip() for l in s[st + 1:end]]
        body = [l for l in body if l and (l.endswith(":") or not l.startswith("."))]           # instructions and labels
        meta = {}
        for l in s[end:end + 400]:
            m = re.match(r"\s*; (\w+)(?::| =) (\d+)", l)
            if m and m.group(1) in META and m.group(1) not in meta:
                meta[m.group(1)] = int(m.group(2))
        out[s[st].split(":")[0]] = (body, meta)
    return out


def counts(body):
    c = collections.Counter(l.split()[0] for l in body if not l.endswith(":"))
    n = lambda *p: sum(v for k, v in c.items() if k.startswith(p))
    return c, {"total": sum(c.values()), "VALU": n("v_") - n("v_mfma"), "MFMA": n("v_mfma"), "DS": n("ds_"),
               "VMEM": n("global_", "buffer_", "scratch_", "flat_"), "SALU": n("s_"), "scratch": n("scratch_")}


def normalised(body):
    """labels renamed to their order of appearance (their numbers shift with every block added or dropped anywhere in the unit)"""
    names = {}
    def label(m):
        return names.setdefault(m.group(0), f".L{len(names)}")
    return [re.sub(r"\.L\w+", label, l) for l in body]


def demangled(names):
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not filt:
        return {n: n for n in names}
    return dict(zip(names, subprocess.run([filt], input="\n".join(names), stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")))


def compare(src, pat, other, defines):
    old, new = kernels(other, src, pat, defines), kernels(B.CSRC, src, pat, defines)
    names = demangled(sorted(set(old) | set(new)))
    same = 0
    for k in sorted(names, key=names.get):
        if k not in old or k not in new:
            print(f"{names[k]}\n  only in {'this tree' if k in new else other}")
            continue
        (bo, mo), (bn, mn) = old[k], new[k]
        co, cn = counts(bo)[1], counts(bn)[1]
        a, b = normalised(bo), normalised(bn)
        if a == b:
            verdict = "identical"
            same += 1
        else:
            sm = difflib.SequenceMatcher(None, a, b, autojunk=False)
            verdict = f"{sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in sm.get_opcodes() if tag != 'equal')} lines differ"
        pair = lambda x, y: f"{x}" if x == y else f"{x} -> {y}"
        print(f"{names[k]}\n  " + "  ".join(f"{m} {pair(mo.get(m), mn.get(m))}" for m in META) + "\n  "
              + "  ".join(f"{m} {co[m]} / {cn[m]}" for m in ("total", "MFMA", "VMEM", "DS")) + f"  {verdict}")
    print(f"{len(names)} kernels, {same} identical")


def main():
    argv = sys.argv[1:]
    defines = [a for a in argv if a.startswith("-D")]
    argv = [a for a in argv if not a.startswith("-D")]
    opt = {}
    for name in ("--top", "--compare"):
        if name in argv:
            i = argv.index(name)
            opt[name] = argv[i + 1]
            del argv[i:i + 2]
    src, pat = argv[0], (argv[1] if len(argv) > 1 else "")
    if "--compare" in opt:
        return compare(src, pat, os.path.abspath(opt["--compare"]), defines)
    top = int(opt.get("--top", 25))
    for name, (body, meta) in kernels(B.CSRC, src, pat, defines).items():
        c, n = counts(body)
        print(f"{name}\n  " + "  ".join(f"{k} {v}" for k, v in n.items()) + f"  {meta}")
        print("  " + "  ".join(f"{k}:{v}" for k, v in c.most_common(top)))


if __name__ == "__main__":
    main()
