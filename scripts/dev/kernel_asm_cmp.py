"""Developer probe (no GPU): compare the device assembly of the kernels two
builds of a step-kernel unit have in common, kernel by kernel -- the
instruction stream and the .amdhsa_ kernel descriptor block (registers, LDS,
scratch) of every kernel whose mangled name contains FILTER (default
step_par_kernel).  A change that only adds instantiations must leave every
earlier one identical; the linked library cannot show that byte for byte,
because the kernels' pc-relative references to their constant tables move
with the layout of the code object, while the assembly names them.

Produce the assembly of a unit with the flags build_ext.py gives it plus
`--cuda-device-only -S`, once per source tree, e.g.

    hipcc --offload-arch=gfx950 -std=c++17 -fPIC -O3 -ffast-math -fno-associative-math \
        -ffp-contract=fast-honor-pragmas -munsafe-fp-atomics -fno-slp-vectorize \
        -mllvm --amdgpu-sched-strategy=iterative-ilp --cuda-device-only -S \
        thormang_isaacgym_amd/csrc/articulation_tree.hip -o new_tree.s

    python scripts/dev/kernel_asm_cmp.py old_tree.s new_tree.s [FILTER]

Exit status 1 when a common kernel differs or one of OLD's is missing in NEW.
"""
import re
import sys


def kernels(path, flt):
    """{kernel: (code lines, descriptor lines)}; the function-local labels
    (.LBB<function index>_<block>) lose the index, which counts the unit's functions."""
    code, desc, cur, mode, funcs = {}, {}, None, None, set()
    for line in open(path):
        t = line.strip()
        m = re.match(r"^\.type\s+(\w+),@function", t)
        if m:   # (a data object's label, a model table with a mangled name, is no kernel)
            funcs.add(m.group(1))
        m = re.match(r"^(\w+):\s*(;.*)?$", t)
        if m and m.group(1) in funcs and mode is None and flt in m.group(1):
            cur, mode = m.group(1), "code"
            code[cur] = []
            continue
        if mode == "code":
            if t.startswith(".Lfunc_end"):
                mode = None
                continue
            t = re.sub(r"\.LBB\d+_", ".LBB_", t)
            t = re.sub(r"\s*;.*$", "", t)
            if t:
                code[cur].append(t)
            continue
        m = re.match(r"^\.amdhsa_kernel\s+(\w+)", t)
        if m and flt in m.group(1):
            cur, mode = m.group(1), "desc"
            desc[cur] = []
            continue
        if mode == "desc":
            if t.startswith(".end_amdhsa_kernel"):
                mode = None
                continue
            desc[cur].append(t)
    return {k: (code[k], desc.get(k)) for k in code}


def main():
    old, new = sys.argv[1], sys.argv[2]
    flt = sys.argv[3] if len(sys.argv) > 3 else "step_par_kernel"
    a, b = kernels(old, flt), kernels(new, flt)
    bad = 0
    for k in sorted(a):
        if k not in b:
            print("MISSING  ", k)
            bad += 1
        elif a[k] != b[k]:
            n = next((i for i, (x, y) in enumerate(zip(a[k][0], b[k][0])) if x != y), None)
            print("DIFFERENT", k, f"{len(a[k][0])} / {len(b[k][0])} instructions, first at {n}",
                  "" if a[k][1] == b[k][1] else "(descriptor too)")
            bad += 1
    added = sorted(set(b) - set(a))
    print(f"{old}: {len(a)} kernels, {sum(len(v[0]) for v in a.values())} lines; {len(a) - bad} identical in {new}, "
          f"{bad} differ or are missing, {len(added)} new")
    for k in added:
        print("new      ", k, len(b[k][0]), "lines")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
