#!/usr/bin/env python3
"""Compare two gfx950 assembly listings function by function.

    hipcc <the flags of mbedtls_amd/build.py> --cuda-device-only -S unit.hip -o a.s
    tools/asm_diff.py a.s b.s [more pairs ...]

A listing is cut at the "-- Begin function" markers; each piece holds one
function's instructions, its .amdhsa_kernel block and its resource comments
(VGPRs, SGPRs, AGPRs, scratch, LDS).  Compiler-local labels carry the
function's ordinal in the file, so they are renumbered in order of first
appearance before the pieces are compared; the code-object metadata at the end
of the file is compared as one more piece.  Prints the functions that differ
or exist on one side only; exit status 1 if there are any.
"""
import re
import sys

BEGIN = re.compile(r"; -- Begin function (\S+)")
LABEL = re.compile(r"\.L(?:BB|func_begin|func_end|JTI|tmp|CPI|__unnamed_)[0-9_]+")
KEYS = ("NumVgprs", "NumAgprs", "TotalNumSgprs", "ScratchSize", "LDSByteSize")


def pieces(path):
    """name -> (is_kernel, normalised lines), in file order"""
    out, name, cur = {}, None, []
    with open(path) as f:
        for line in f:
            m = BEGIN.search(line)
            meta = line.lstrip().startswith(".amdgpu_metadata")
            if m or meta:
                if name is not None:
                    out[name] = cur
                name, cur = (m.group(1) if m else "<amdgpu_metadata>"), []
            if name is not None and "@object" in line and line.lstrip().startswith(".type"):
                out[name] = cur    # the unit's data objects follow its last function
                name = None
            if name is None or line.lstrip().startswith((".section", ".file", ".ident")):
                continue   # .section names the *next* function: order, not code
            cur.append(line.rstrip())
    if name is not None:
        out[name] = cur
    res = {}
    for name, lines in out.items():
        ids = {}
        text = [LABEL.sub(lambda m: ids.setdefault(m.group(0), ".L%d" % len(ids)), l) for l in lines]
        res[name] = (any(".amdhsa_kernel" in l for l in lines), text)
    return res


def resources(lines):
    got = {}
    for l in lines:
        for k in KEYS:
            if l.startswith("; " + k + ":"):
                got[k] = l.split(":", 1)[1].split()[0]
    return " ".join("%s=%s" % (k, got.get(k, "?")) for k in KEYS)


def compare(pa, pb):
    a, b = pieces(pa), pieces(pb)
    bad = 0
    for name in list(a) + [n for n in b if n not in a]:
        if name not in a or name not in b:
            print("  only in %s: %s" % (pb if name in b else pa, name))
            bad += 1
        elif a[name][1] != b[name][1]:
            la, lb = a[name][1], b[name][1]
            first = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
            print("  differs: %s\n    %d / %d lines, first at %d\n    a: %s\n    b: %s"
                  % (name, len(la), len(lb), first, resources(la), resources(lb)))
            bad += 1
    kernels = sum(1 for n in a if a[n][0])
    print("%s %s: %d kernels, %d functions, %s" % (pa, pb, kernels, len(a) - kernels - ("<amdgpu_metadata>" in a),
                                                   "identical: all" if not bad else "%d differ" % bad))
    return bad, kernels


def main(argv):
    if len(argv) < 2 or len(argv) % 2:
        sys.exit(__doc__)
    bad = total = 0
    for i in range(0, len(argv), 2):
        d, k = compare(argv[i], argv[i + 1])
        bad += d
        total += k
    if len(argv) > 2:
        print("total: %d kernels, %s" % (total, "identical: all" if not bad else "%d pieces differ" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
