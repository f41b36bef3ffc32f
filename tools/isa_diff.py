#!/usr/bin/env python3
"""Same machine code?  usage: isa_diff.py OLD_TREE NEW_TREE [--pair OLD_SUBSTRING=NEW_SUBSTRING]...

Compiles every raytracer3_amd/csrc/*.hip of both trees with that tree's own Makefile FLAGS plus `--cuda-device-only -S` (no GPU needed) and
compares, per mangled symbol and whichever file it came from: each function's instruction text, a kernel's .amdhsa_* descriptor block and
`.set <symbol>.*` resource lines, its entry in the code object's metadata (registers, scratch, LDS, kernarg size, arguments) and every device
global (the __constant__ knobs included) with its section and initial value.  Only what depends on a function's position in its translation
unit is normalised: .LBB<n>_<m>, .Lfunc_begin<n> / .Lfunc_end<n>, .file / .ident lines and assembler comments; the per-file __hip_cuid_<hash>
marker is left out.  Texts are compared whole.  Symbols that differ or exist on one side only go to stdout (nothing when there are none),
the closing count to stderr; the exit status is 1 if anything was printed.

--pair (repeatable) is for a renamed kernel: the one kernel only in OLD whose mangled name contains OLD_SUBSTRING and the one only in NEW
whose name contains NEW_SUBSTRING are compared with each other instead of being listed as "only in": registers, LDS, scratch and kernarg
bytes, the global loads and stores by width, and every opcode whose count differs.  A pair is a report, not a difference: it does not
count towards the exit status."""
import collections
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


def kernel_summary(tree, name):
    """(resource fields of the metadata entry, opcode counts of the code) of one kernel"""
    meta, code = tree[name, "metadata"][0], tree[name, "code"][0]
    fields = {f: int(re.search(r"\.%s:\s+(\d+)" % f, meta).group(1))
              for f in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "kernarg_segment_size")}
    lines = (line.split() for line in code.split("\n")[1:])
    return fields, collections.Counter(t[0] for t in lines if t and not t[0].startswith(".") and not t[0].endswith(":"))


def report_pair(old, new, spec):
    """prints the comparison of the pair named by `spec`; returns the two mangled names"""
    names = []
    for tree, other, sub in zip((old, new), (new, old), spec.split("=", 1)):
        hit = [n for n, part in tree if part == "descriptor" and sub in n and (n, part) not in other]
        if len(hit) != 1:
            sys.exit("isa_diff: --pair %s: %r matches %d kernels that are on one side only: %s" % (spec, sub, len(hit), hit))
        names += hit
    (fo, oo), (fn, on) = kernel_summary(old, names[0]), kernel_summary(new, names[1])
    print("pair:        %s -> %s" % tuple(names))
    print("  " + ", ".join("%s %d -> %d" % (f, fo[f], fn[f]) for f in fo))
    memory = sorted(op for op in set(oo) | set(on) if re.match(r"(global|flat|buffer|scratch)_(load|store)", op))
    print("  memory: " + (", ".join("%s %d -> %d" % (op, oo[op], on[op]) for op in memory) or "none"))
    other = sorted(op for op in set(oo) | set(on) if oo[op] != on[op] and op not in memory)
    print("  instructions %d -> %d; counts that differ: " % (sum(oo.values()), sum(on.values()))
          + (", ".join("%s %d -> %d" % (op, oo[op], on[op]) for op in other) or "none"))
    return names


def main():
    args, pairs = sys.argv[1:], []
    while "--pair" in args[:-1]:
        pairs.append(args.pop(args.index("--pair") + 1))
        args.remove("--pair")
    if len(args) != 2 or any("=" not in p for p in pairs):
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b:
        old, new = tree_symbols(args[0], a), tree_symbols(args[1], b)
    for names in [report_pair(old, new, p) for p in pairs]:
        for tree, name in zip((old, new), names):
            for key in [k for k in tree if k[0] == name]:
                del tree[key]
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
