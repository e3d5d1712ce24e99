"""Do two trees compile to the same kernels?  python tools/kernel_asm_diff.py OLD_TREE NEW_TREE > profiles/<name>.txt

Compiles every .hip translation unit of both trees to gfx950 assembly with the flags that tree's pyctcdecode_amd/build.py gives the
file (plus --cuda-device-only -S), cuts the output per kernel symbol -- the body up to its end label and the .amdhsa_ descriptor
block -- and compares kernel by kernel, wherever in the tree a kernel lives: a refactor that moves kernels between files, or
touches only host code, must leave every line `identical`. Comments and .loc / .file lines are dropped, and local labels are
renumbered in order of appearance (.LBB<function>_<n> carries the function's index in its file). One line per kernel:
identical, differs, missing (only in OLD_TREE), new (only in NEW_TREE) or duplicate (emitted by more than one file of a tree).
Exit status 1 unless every kernel is identical."""
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor


def load_build(tree):
    path = os.path.join(tree, "pyctcdecode_amd", "build.py")
    spec = importlib.util.spec_from_file_location("build_" + str(abs(hash(path))), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def assembly(build, src, out):
    cmd = build._compile_cmd(src, out)
    i = cmd.index("-c")
    cmd[i:i + 1] = ["--cuda-device-only", "-S"]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(out) as f:
        return f.read().splitlines()


LOCAL = re.compile(r"\.L[A-Za-z_]+[0-9][0-9_]*")


def clean(lines):
    """Comments, debug-line directives and blank lines out; local labels renumbered in order of appearance."""
    names, out = {}, []
    for line in lines:
        line = line.split(";", 1)[0].strip()
        if not line or line.startswith((".loc", ".file")):
            continue
        line = LOCAL.sub(lambda m: names.setdefault(m.group(0), ".L%d" % len(names)), line)
        out.append(" ".join(line.split()))
    return out


def kernels(lines):
    """{symbol: cleaned body + descriptor} of one assembly file."""
    desc, k = {}, 0
    while k < len(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", lines[k])
        if m:
            end = next(j for j in range(k, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
            desc[m.group(1)] = lines[k + 1:end]
            k = end
        k += 1
    found = {}
    for sym, d in desc.items():
        start = next(j for j, line in enumerate(lines) if line.startswith(sym + ":"))
        end = next(j for j in range(start, len(lines)) if lines[j].startswith(".Lfunc_end"))
        # (resource symbols the descriptor may be written in terms of: `.set <symbol>.<what>, <value>`)
        sets = [line for line in lines if line.strip().startswith(".set " + sym + ".")]
        found[sym] = clean(lines[start + 1:end]) + ["--"] + clean(sets) + ["--"] + clean(d)
    return found


def tree_kernels(tree, tmp, tag):
    build = load_build(tree)
    srcs = [s for s in build.SOURCES if s.endswith(".hip")]
    with ThreadPoolExecutor(max(1, min(len(srcs), os.cpu_count() or 1))) as ex:
        texts = list(ex.map(lambda s: assembly(build, s, os.path.join(tmp, tag + "_" + s + ".s")), srcs))
    where = {}  # symbol -> [(file, text)]
    for src, text in zip(srcs, texts):
        for sym, body in kernels(text).items():
            where.setdefault(sym, []).append((src, body))
    return where


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        old = tree_kernels(sys.argv[1], tmp, "old")
        new = tree_kernels(sys.argv[2], tmp, "new")
    syms = sorted(set(old) | set(new))
    plain = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True).stdout.splitlines()
    counts = {}
    for sym, name in zip(syms, plain):
        o, n = old.get(sym, []), new.get(sym, [])
        if len(o) > 1 or len(n) > 1:
            verdict = "duplicate"
        elif not n:
            verdict = "missing"
        elif not o:
            verdict = "new"
        else:
            verdict = "identical" if o[0][1] == n[0][1] else "differs"
        counts[verdict] = counts.get(verdict, 0) + 1
        files = "%s -> %s" % ("+".join(f for f, _ in o) or "-", "+".join(f for f, _ in n) or "-")
        print("%-9s  %-44s  %s" % (verdict, files, name))
    print("# %d kernels: %s" % (len(syms), ", ".join("%d %s" % (c, v) for v, c in sorted(counts.items()))))
    sys.exit(0 if set(counts) <= {"identical"} else 1)


if __name__ == "__main__":
    main()
