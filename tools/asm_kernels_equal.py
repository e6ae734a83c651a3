"""Are two device-only assembly files (hipcc --offload-arch=gfx950 --cuda-device-only -S) the same kernels?

usage: python tools/asm_kernels_equal.py parent.s branch.s
       python tools/asm_kernels_equal.py parent_dir branch_dir      (every x.s with kernels in parent_dir against branch_dir/x.s)

A host-side refactor that touches no __global__ function may still change the ORDER in which templated kernels are
instantiated, and with it the order of the functions in the .s file and the function index in every local label
(.LBB<index>_<n>, .Lfunc_end<index>): a plain diff is then large although no instruction moved.  This compares the files
function by function, by mangled name, with that index taken out of the labels; everything else must be identical,
the kernel descriptors and metadata (compared as sorted blocks) included.  Exit status 0: same kernels."""
import os
import re
import sys


def functions(path):
    text = open(path).read()
    head, _, meta = text.partition("\t.amdgpu_metadata")
    head = head.split("\t.text\n\t.p2alignl 6,")[0]            # (the file's trailer: padding, compile-unit id, .ident)
    parts = re.split(r"(?m)^(?=\t\.section\t\.text\.)", head)
    fns = {}
    for p in parts[1:]:
        name = re.match(r"\t\.section\t\.text\.([^,]+),", p).group(1)
        body = re.sub(r"(?m)^.*__hip_cuid_.*\n", "", p)                              # (compile-unit id: a hash of the source file)
        body = re.sub(r"(?m)\s*;.*$", "", body)                                        # (comments name blocks by that index too)
        body = re.sub(r"\.(LBB|Lfunc_end|Lfunc_begin|L__unnamed_|Ltmp)\d+", r".\1#", body)
        fns[name] = fns.get(name, "") + body         # (a function's text and its descriptor are two sections of one name)
    kernels = sorted(re.findall(r"(?ms)^  - \.agpr_count:.*?(?=^  - \.agpr_count:|^amdhsa\.|\Z)", meta))
    return fns, kernels


def main(a, b):
    fa, ka = functions(a)
    fb, kb = functions(b)
    bad = sorted(set(fa) ^ set(fb)) + [n for n in fa if n in fb and fa[n] != fb[n]]
    print("%d / %d functions, %d differ or are missing; metadata blocks %s" %
          (len(fa), len(fb), len(bad), "equal" if ka == kb else "DIFFER"))
    for n in bad[:20]:
        print("  ", n)
    return 1 if bad or ka != kb or not fa else 0


if __name__ == "__main__":
    a, b = sys.argv[1:3]
    if os.path.isdir(a):
        names = [n for n in sorted(os.listdir(a)) if n.endswith(".s") and ".amdhsa_kernel" in open(os.path.join(a, n)).read()]
        rcs = [print(n, end=": ") or main(os.path.join(a, n), os.path.join(b, n)) for n in names]      # (files without kernels: skipped)
        sys.exit(1 if any(rcs) or not rcs else 0)
    sys.exit(main(a, b))
