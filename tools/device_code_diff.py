#!/usr/bin/env python3
"""Are the gfx950 code objects of two checkouts the same device code?  (no GPU needed)

    python tools/device_code_diff.py <checkout A> <checkout B>
    python tools/device_code_diff.py --kernels-of-a <checkout A> <checkout B>
    python tools/device_code_diff.py --union <checkout A> <checkout B>

Per csrc/*.hip translation unit: the device-only compile line of tools/kernel_resources.py, clang-offload-bundler
--unbundle, then `llvm-objdump -d` (without its file-name lines) and `llvm-readelf --notes` of both code objects.  Two
builds of one source differ in a few bytes of the object file, but not in these two texts: equal texts mean the same
kernels under the same names with the same instructions, registers, LDS and scratch.  Prints `equal` per translation
unit, or the first kernel whose instructions or metadata differ; exits 1 if anything differs.

--kernels-of-a: for a checkout B that ADDS kernels to A (a new conv family), where the whole texts cannot be equal: every symbol of
A's disassembly is looked up by name in B's and its instructions compared with the addresses taken out (the symbol's own address
and the `// address:` column; encodings stay), and every kernel of A's metadata note is compared with B's of the same name.  Prints
per translation unit how many of A's kernels B holds unchanged and how many it adds; exits 1 if one of A's is missing or differs.

--union: for a checkout B that MOVES launch sites between translation units.  The kernels are `static __global__` in a header, so a unit
holds the code of exactly the kernels it launches and a moved launch site moves the code with it: the per-unit texts cannot be equal.
Units whose two texts are equal still print `equal`.  Then, over all units together: every symbol and every kernel note of A, in every
distinct form it has in A, must be in some unit of B under the same name with the same instructions (addresses taken out as above) and
the same metadata, and B must name nothing that A does not; exits 1 otherwise.
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
SYMBOL, SYMBOL_NAME = r"(?m)^(?=[0-9a-f]+ <)", r"^[0-9a-f]+ <([^>]+)>:"      # a symbol of the disassembly
NOTE, NOTE_NAME = r"(?m)^(?=\s+- \.agpr_count:)", r"\.name:\s+(\S+)"          # a kernel of the metadata note


def start(root, tmp):
    csrc = os.path.join(root, "cmf.jl_amd", "csrc")
    jobs = {}
    for src in sorted(f for f in os.listdir(csrc) if f.endswith(".hip")):
        obj = os.path.join(tmp, src + ".o")
        jobs[src] = (obj, subprocess.Popen(["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-c", "--cuda-device-only",
                                            "-I", os.path.join(root, "include"), "-I", csrc, os.path.join(csrc, src), "-o", obj]))
    return jobs


def texts(src, obj, proc):
    if proc.wait() != 0:
        raise RuntimeError(f"hipcc failed on {src}")
    co = obj + ".co"
    subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={obj}",
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"])
    dis = subprocess.check_output([f"{LLVM}/llvm-objdump", "-d", co]).decode()
    dis = "\n".join(ln for ln in dis.split("\n") if co not in ln)  # the file-name lines
    return dis, subprocess.check_output([f"{LLVM}/llvm-readelf", "--notes", co]).decode()


def demangle(name):
    try:
        return subprocess.run(["c++filt", name], stdout=subprocess.PIPE).stdout.decode().strip() or name
    except OSError:
        return name


def by_name(text, split, name_of, strip_addresses):
    """{name: block} of the blocks of `split`; strip_addresses: without the symbol's address and the address column of every line."""
    out = {}
    for blk in re.split(split, text)[1:]:
        name = re.search(name_of, blk).group(1)
        if strip_addresses:
            blk = re.sub(r"(?m)^[0-9a-f]+ (<[^>]+>:)", r"\1", re.sub(r"// [0-9A-Fa-f]+:", "//", blk))
        # what follows the LAST block of a text belongs to the file, not to the block: objdump's `...` for the padding behind the last
        # symbol, the note's closing lines (amdhsa.target, amdhsa.version) behind the last kernel
        blk = re.sub(r"(?m)^amdhsa\.target:(.|\n)*", "", blk).rstrip()
        out[name] = re.sub(r"\n\s*\.\.\.$", "", blk).rstrip()
    return out


def kernels_of_a(src, da, na, db, nb):
    """True when every symbol and every kernel note of A is in B unchanged."""
    bad = []
    for what, a, b in (("instructions", by_name(da, SYMBOL, SYMBOL_NAME, True), by_name(db, SYMBOL, SYMBOL_NAME, True)),
                       ("metadata", by_name(na, NOTE, NOTE_NAME, False), by_name(nb, NOTE, NOTE_NAME, False))):
        missing = [k for k in a if k not in b]
        changed = [k for k in a if k in b and a[k] != b[k]]
        for k in missing + changed:
            bad.append(f"{src}: {what} of {demangle(k)} {'missing' if k in missing else 'differ'}")
        if what == "metadata":
            print(f"{src}: {len(a) - len(missing) - len(changed)} of A's {len(a)} kernels unchanged in B, {len(b) - len(a) + len(missing)} added"
                  + ("" if not bad else f", {len(bad)} differences"))
    for line in bad[:20]:
        print(line)
    return not bad


def union(texts_a, texts_b):
    """--union.  texts_*: {translation unit: (disassembly, notes)}.  True when every block of A is in some unit of B and B names nothing new."""
    ok = True
    for src in sorted(set(texts_a) | set(texts_b)):
        a, b = texts_a.get(src), texts_b.get(src)
        n = [len(re.findall(r"\.agpr_count:", t[1])) if t else 0 for t in (a, b)]
        print(f"{src}: " + (f"equal ({n[0]} kernels)" if a == b else f"{n[0]} kernels in A, {n[1]} in B: compared in the union"))
    for what, split, name_of, strip, which in (("instructions", SYMBOL, SYMBOL_NAME, True, 0), ("metadata", NOTE, NOTE_NAME, False, 1)):
        all_a, all_b = {}, {}
        for texts, out in ((texts_a, all_a), (texts_b, all_b)):
            for src, t in texts.items():
                for name, blk in by_name(t[which], split, name_of, strip).items():
                    out.setdefault(name, {}).setdefault(blk, src)
        lost = [(k, src) for k, blks in all_a.items() for blk, src in blks.items() if blk not in all_b.get(k, {})]
        added = [k for k in all_b if k not in all_a]
        print(f"union, {what}: {sum(len(v) for v in all_a.values())} distinct blocks under {len(all_a)} names in A, "
              f"{sum(len(v) for v in all_b.values())} under {len(all_b)} in B; {len(lost)} of A's not in B, {len(added)} names added")
        for k, src in lost[:20]:
            print(f"  {what} of {demangle(k)} ({src} of A) {'differ' if k in all_b else 'missing'} in B")
        for k in added[:20]:
            print(f"  {what} of {demangle(k)} only in B")
        ok &= not lost and not added
    return ok


def first_difference(a, b, split, name_of):
    """The name of the first block (of `split`) that differs between the two texts."""
    for x, y in zip(re.split(split, a), re.split(split, b)):
        if x != y:
            m = re.search(name_of, x) or re.search(name_of, y)
            return demangle(m.group(1)) if m else "(before the first kernel)"
    return "(one text is a prefix of the other: a kernel was added or removed at the end)"


if __name__ == "__main__":
    per_kernel, over_all = "--kernels-of-a" in sys.argv, "--union" in sys.argv
    for flag in ("--kernels-of-a", "--union"):
        if flag in sys.argv:
            sys.argv.remove(flag)
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    differ = False
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        ja, jb = start(sys.argv[1], ta), start(sys.argv[2], tb)
        if over_all:
            sys.exit(0 if union({s: texts(s, *j) for s, j in ja.items()}, {s: texts(s, *j) for s, j in jb.items()}) else 1)
        for src in sorted(set(ja) | set(jb)):
            if src not in ja or src not in jb:
                print(f"{src}: only in {sys.argv[1] if src in ja else sys.argv[2]}")
                differ = True
                continue
            (da, na), (db, nb) = texts(src, *ja[src]), texts(src, *jb[src])
            if per_kernel:
                differ |= not kernels_of_a(src, da, na, db, nb)
                continue
            n_kernels = len(re.findall(r"\.agpr_count:", na))
            if da == db and na == nb:
                print(f"{src}: equal ({n_kernels} kernels, {da.count(chr(10))} lines of disassembly, {na.count(chr(10))} lines of notes)")
                continue
            differ = True
            if da != db:
                print(f"{src}: instructions differ, first in {first_difference(da, db, SYMBOL, SYMBOL_NAME)}")
            if na != nb:
                print(f"{src}: metadata differs, first in {first_difference(na, nb, NOTE, NOTE_NAME)}")
    sys.exit(1 if differ else 0)
