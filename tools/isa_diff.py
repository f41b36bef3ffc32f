#!/usr/bin/env python3
"""Same machine code?  usage: isa_diff.py OLD_TREE NEW_TREE

Compiles every raytracer3_amd/csrc/*.hip of both trees with that tree's own Makefile FLAGS plus `--cuda-device-only -S` (no GPU needed) and
compares, per mangled symbol and whichever file it came from: each function's instruction text, a kernel's .amdhsa_* descriptor block and
`.set <symbol>.*` resource lines, its entry in the code object's metadata (registers, scratch, LDS, kernarg size, arguments) and every device
global (the __constant__ knobs included) with its section and initial value.  Only what depends on a function's position in its translation
unit is normalised: .LBB<n>_<m>, .Lfunc_begin<n> / .Lfunc_end<n>, .file / .ident lines and assembler comments; the per-file __hip_cuid_<hash>
marker is left out.  Texts are compared whole.  Symbols that differ or exist on one side only go to stdout (nothing when there are none),
the closing count to stderr; the exit status is 1 if anything was printed."""
import concurrent.futures
import glob
import os
import re
import subprocess
import sys
import tempfile

CSRC = os.path.join("raytracer3_amd", "csrc")


def normalise(text):
    out = []
    for line in text.split("\n"):
        if '"' not in line:
            line = line.split(";", 1)[0]
        line = line.rstrip()
        if not line or re.match(r"\s*\.(file|ident)\b", line):
            continue
        line = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", line)
        out.append(re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", line))
    return "\n".join(out)


def symbols_of(asm):
    """{(symbol, part): text} of one normalised assembly file."""
    code, _, meta = asm.partition("\t.amdgpu_metadata")
    found = {}
    for name in re.findall(r"^\s*\.type\s+(\S+),@function$", code, re.M):
        q = re.escape(name)
        found[name, "code"] = re.search(r"^%s:$.*?^\.Lfunc_end:$" % q, code, re.M | re.S).group(0)
        found[name, "set"] = "\n".join(re.findall(r"^\s*\.set %s\..*$" % q, code, re.M))
        kd = re.search(r"^\s*\.amdhsa_kernel %s$.*?^\s*\.end_amdhsa_kernel$" % q, code, re.M | re.S)
        if kd:
            found[name, "descriptor"] = kd.group(0)
    for name in re.findall(r"^\s*\.type\s+(\S+),@object$", code, re.M):
        if not name.startswith("__hip_cuid_"):
            q = re.escape(name)
            found[name, "global"] = re.search(r"^\s*\.type\s+%s,@object$.*?^\s*\.size\s+%s, \d+$" % (q, q), code, re.M | re.S).group(0)
    for line in re.findall(r"^\s*\.amdgpu_lds .*$", code, re.M):
        found[line.split()[1].rstrip(","), "lds"] = line
    kernels = meta.partition("amdhsa.kernels:\n")[2].partition("\namdhsa.target:")[0]
    for entry in re.split(r"^  - ", kernels, flags=re.M)[1:]:
        found[re.search(r"\.name:\s+(\S+)", entry).group(1), "metadata"] = entry.rstrip()
    return found


def tree_symbols(tree, tmp):
    csrc = os.path.join(tree, CSRC)
    cmd = subprocess.run(["make", "-s", "--no-print-directory", "-C", csrc, "--eval", "isa-diff-flags: ; @echo $(HIPCC) $(FLAGS)", "isa-diff-flags"], check=True,
                         capture_output=True, text=True).stdout.split()

    def compile_one(src):
        out = os.path.join(tmp, os.path.basename(src)[:-4] + ".s")
        subprocess.run(cmd + ["--cuda-device-only", "-S", os.path.basename(src), "-o", out], cwd=csrc, check=True, capture_output=True)
        return symbols_of(normalise(open(out).read()))

    merged = {}  # a symbol defined in several files (a device function of a shared header) keeps all its texts, sorted
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        for found in pool.map(compile_one, sorted(glob.glob(os.path.join(csrc, "*.hip")))):
            for key, text in found.items():
                merged.setdefault(key, []).append(text)
    return {key: sorted(texts) for key, texts in merged.items()}


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b:
        old, new = tree_symbols(sys.argv[1], a), tree_symbols(sys.argv[2], b)
    bad = 0
    for name, part in sorted(set(old) | set(new)):
        if (name, part) not in new:
            print("only in OLD:", part, name)
        elif (name, part) not in old:
            print("only in NEW:", part, name)
        elif old[name, part] != new[name, part]:
            print("differs:    ", part, name)
        else:
            continue
        bad += 1
    kernels = lambda t: sum(1 for _, part in t if part == "descriptor")
    print("isa_diff: %d kernels and %d symbol texts in OLD, %d and %d in NEW, %d differ or are on one side only"
          % (kernels(old), len(old), kernels(new), len(new), bad), file=sys.stderr)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
