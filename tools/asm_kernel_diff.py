#!/usr/bin/env python3
"""Compare the kernels of two device-assembly files (hipcc -S --cuda-device-only) one by one:
per kernel of the first file, the lines that differ in the second after dropping comments and
the per-function numbers of local labels (.LBB<n>_, .Lfunc_end<n>) -- those numbers shift when a
kernel is added to the translation unit, the instructions do not.
usage: asm_kernel_diff.py OLD.s NEW.s [--show N]"""
import difflib
import re
import sys


def kernels(path):
    out, cur = {}, None
    for ln in open(path):
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            cur = m.group(1)
            out[cur] = []
        if cur is not None:
            code = re.sub(r"(\.LBB|\.Lfunc_end|\.Lfunc_begin)\d+", r"\1N", ln.split(";")[0].rstrip())
            if code:
                out[cur].append(code)
        if ln.startswith(".Lfunc_end"):
            cur = None
    return out


def main():
    show = int(sys.argv[sys.argv.index("--show") + 1]) if "--show" in sys.argv else 40
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    rc = 0
    for k in a:
        if k not in b:
            print("%s: %d lines, gone" % (k, len(a[k])))
            rc = 1
            continue
        d = [l for l in difflib.unified_diff(a[k], b[k], n=0, lineterm="") if l[:3] not in ("---", "+++")]
        print("%s: %d lines, %d diff lines" % (k, len(a[k]), len(d)))
        for l in d[:show]:
            print("  " + l)
        rc |= bool(d)
    for k in b:
        if k not in a:
            print("%s: %d lines, new" % (k, len(b[k])))
    return rc


if __name__ == "__main__":
    sys.exit(main())
