"""Compare two hipcc -S outputs of one source file, kernel by kernel:

    python scripts/asm_compare.py parent.s new.s
    python scripts/asm_compare.py parent.s new_a.s,new_b.s    (a side may be several files: kernels that moved)

For every kernel of the first file: whether the second has it, and whether its instruction stream
(labels normalised, comments dropped) and its resources (.amdhsa_* lines: registers, LDS, scratch,
kernarg size) are the same; differing lines are printed. Kernels only the second file has are listed.
Exit status 1 if a kernel of the first file is missing from the second."""
import difflib
import re
import subprocess
import sys


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def kernels(path):
    """name -> (instructions, {resource: value}) of every .amdhsa_kernel in the file"""
    lines = open(path).read().split("\n")
    names = [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")]
    out = {}
    for name in names:
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        body, res, labels = [], {}, {}
        i = start + 1
        while not lines[i].startswith(".Lfunc_end"):
            l = lines[i].split(";")[0].rstrip()
            s = l.strip()
            if s.startswith(".amdhsa_") and not s.startswith(".amdhsa_kernel"):
                k, _, v = s.partition(" ")
                res[k] = v.strip()
            elif s and (not s.startswith(".") or s.startswith(".LBB")):
                body.append(s)
            i += 1
        for l in body:  # labels by order of definition
            if l.startswith(".LBB") and l.endswith(":"):
                labels[l[:-1]] = f".L{len(labels)}"
        rx = re.compile(r"\.LBB\d+_\d+")
        out[name] = ([rx.sub(lambda m: labels.get(m.group(0), m.group(0)), l) for l in body], res)
    return out


def key(demangled):
    """(name, template arguments) of a demangled kernel, without its argument list"""
    head = demangled.split("(anonymous namespace)::", 1)[-1].split("(")[0]
    name, _, targs = head.partition("<")
    return name.split()[-1], [t.strip() for t in targs.rstrip(">").split(",") if t.strip()]


def same_kernel(kt, bt):
    """bt is kt, or kt followed by template parameters the second file added at their defaults"""
    return bt[:len(kt)] == kt and all(t in ("false", "0") for t in bt[len(kt):])


def table(files):
    """--table: per kernel of each file, its size and resources as one markdown table"""
    for path in files:
        ks = kernels(path)
        dm = demangle(sorted(ks))
        print(f"\n### {path}\n")
        print("| kernel | instructions | conditional branches | VGPRs | private segment (B) |")
        print("|---|---:|---:|---:|---:|")
        for n in sorted(ks, key=lambda n: dm[n]):
            kn, kt = key(dm[n])
            body, res = ks[n]
            ins = [l for l in body if not l.endswith(":")]
            cbr = sum(1 for l in ins if l.split()[0].startswith("s_cbranch"))
            print(f"| `{kn}<{','.join(kt)}>` | {len(ins)} | {cbr} | {res.get('.amdhsa_next_free_vgpr')} | "
                  f"{res.get('.amdhsa_private_segment_fixed_size')} |")


def main():
    if sys.argv[1] == "--table":
        table(sys.argv[2:])
        return 0
    a, b = ({n: k for path in side.split(",") for n, k in kernels(path).items()} for side in sys.argv[1:3])
    dm = demangle(sorted(set(a) | set(b)))
    bkeys = {n: key(dm[n]) for n in b}
    missing = 0
    matched = set()
    for pname in a:
        print(f"== {dm[pname]}")
        kn, kt = key(dm[pname])
        name = next((n for n, (bn, bt) in bkeys.items() if bn == kn and same_kernel(kt, bt)), None)
        if name is None:
            print("   MISSING from the second file")
            missing += 1
            continue
        matched.add(name)
        (ia, ra), (ib, rb) = a[pname], b[name]
        d = [l for l in difflib.unified_diff(ia, ib, lineterm="", n=0) if not l.startswith(("---", "+++", "@@"))]
        print(f"   instructions: {len(ia)} -> {len(ib)}: " + ("identical" if not d else f"{len(d)} differing lines"))
        for l in d[:40]:
            print("     " + l)
        dr = {k: (ra.get(k), rb.get(k)) for k in sorted(set(ra) | set(rb)) if ra.get(k) != rb.get(k)}
        print("   resources: " + ("identical" if not dr else ", ".join(f"{k[8:]} {v[0]} -> {v[1]}" for k, v in dr.items())))
    new = [n for n in b if n not in matched]
    print(f"== {len(new)} kernels only in the second file")
    for n in new:
        r = b[n][1]
        print(f"   {dm[n]}: {len(b[n][0])} instructions, vgpr {r.get('.amdhsa_next_free_vgpr')}, sgpr {r.get('.amdhsa_next_free_sgpr')}, "
              f"LDS {r.get('.amdhsa_group_segment_fixed_size')}, scratch {r.get('.amdhsa_private_segment_fixed_size')}")
    return 1 if missing else 0


if __name__ == "__main__":
    raise SystemExit(main())
