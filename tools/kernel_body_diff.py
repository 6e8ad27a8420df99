#!/usr/bin/env python3
"""Are a kernel template's instantiations the same machine code in two builds of one source file?

    hipcc <the Makefile's FLAGS> --offload-device-only -S before/mke_sampler.hip -o before.s     (likewise after.s)
    python tools/kernel_body_diff.py before.s <the template's name before> after.s k_neg_sample

Takes two device-assembly listings and, for each, the name of a kernel template in namespace mke.  Instantiations are paired by
their template arguments; a body is the text from the kernel's label to its s_endpgm.  Symbol names are set aside: the mangled
name, and the ordinal of the function inside its file that every local label (.LBB<ordinal>_<block>) carries.  Prints the
template arguments, both line counts and the verdict per instantiation; exit status 1 if any body differs or has no partner."""
import re
import sys


def bodies(path, kernel):
    """{template arguments as mangled: body lines} of the instantiations of mke::<kernel> in the listing."""
    head = re.compile(r"^(_ZN3mke%d%sI(\w+?)EEv\w+):" % (len(kernel), re.escape(kernel)))
    out, cur = {}, None
    for line in open(path):
        m = head.match(line)
        if m and cur is None:
            cur, buf = m.group(2), []
        elif cur is not None:
            buf.append(line)
            if line.strip().startswith("s_endpgm"):
                out[cur], cur = buf, None
    return out


def normalised(lines):
    return [re.sub(r"\s+;", " ;", re.sub(r"BB\d+_", "BB_", re.sub(r"_ZN3mke\w+", "SYM", l))) for l in lines]


def main(argv):
    if len(argv) != 4:
        sys.exit(__doc__)
    a, b = bodies(argv[0], argv[1]), bodies(argv[2], argv[3])
    bad = 0
    for args in sorted(set(a) | set(b)):
        if args not in a or args not in b:
            print(f"<{args}>  only in {'the first' if args in a else 'the second'} listing")
            bad += 1
            continue
        x, y = normalised(a[args]), normalised(b[args])
        same = x == y
        bad += not same
        print(f"<{args}>  {len(x)} / {len(y)} lines  " + ("identical" if same else f"DIFFERENT ({sum(p != q for p, q in zip(x, y)) + abs(len(x) - len(y))} lines)"))
    print(f"{len(set(a) | set(b))} instantiations, {bad} not identical")
    return 1 if bad or not a else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
