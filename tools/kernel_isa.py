"""Device code of a tree, one text file per function, so that two trees can be compared with `diff -r`.
Usage: kernel_isa.py <tree root> <output dir>

Every translation unit of the tree (UNITS of its staticmapping_amd/build.py; HIP_SOURCES in trees that predate the per-unit
build) is compiled with the build's own flags plus --cuda-device-only -S.  For each function of the assembly -- the kernels
and the device functions they call out of line -- <output dir>/<mangled name>.s holds its instructions with comments stripped
and the labels that number functions within a module (.LBB<n>_, .Lfunc_end<n>) normalised; a kernel's file ends with its
.amdhsa_ resource lines (VGPRs, SGPRs, LDS, scratch, ...).  Which unit a function was compiled in is not recorded: moving a
kernel between units leaves the output unchanged exactly when its code is."""
import hashlib
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor


def units_of(tree):
    spec = importlib.util.spec_from_file_location("_tree_build", os.path.join(tree, "staticmapping_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return [u for u in getattr(b, "UNITS", None) or b.HIP_SOURCES if u.endswith(".hip")]


def assembly(tree, unit, tmp):
    out = os.path.join(tmp, unit + ".s")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", "include", "-Wno-unused-command-line-argument",
                           "--cuda-device-only", "-S", "-o", out, os.path.join("staticmapping_amd", "csrc", unit)], cwd=tree)
    return open(out).read().splitlines()


def functions(lines):
    """{name: normalised text} of one module's assembly."""
    found, name, body, res = {}, None, [], []
    for raw in lines:
        line = raw.split(";")[0].strip()
        m = re.match(r"\.type\s+(\S+),@function", line)
        if m:
            name, body, res, in_code = m.group(1), [], [], False
        elif name is None or not line:
            continue
        elif line == name + ":":
            in_code = True
        elif line.startswith(".Lfunc_end"):
            found[name] = "\n".join(body + res) + "\n"
            name = None
        elif line.startswith(".amdhsa_") and not line.startswith(".amdhsa_kernel"):
            res.append(line)
        elif line.startswith(".section"):
            in_code = False                     # the kernel descriptor follows the last instruction
        elif in_code:
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", line)))
    return found


def main(tree, out_dir):
    os.makedirs(out_dir, exist_ok=True)
    units = units_of(tree)
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as pool:
        modules = list(pool.map(lambda u: functions(assembly(tree, u, tmp)), units))
    seen = {}
    for unit, fns in zip(units, modules):
        for name, text in fns.items():
            if seen.setdefault(name, (unit, text))[1] != text:      # (library templates may be instantiated in several units)
                sys.exit(f"{name}: different code in {seen[name][0]} and {unit}")
    for name, (_, text) in seen.items():
        fname = name if len(name) <= 200 else name[:160] + "." + hashlib.sha1(name.encode()).hexdigest()
        with open(os.path.join(out_dir, fname + ".s"), "w") as fh:
            fh.write(text)
    print(f"{len(seen)} functions of {len(units)} units, {sum('.amdhsa_' in t for _, t in seen.values())} of them kernels")


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]), sys.argv[2])
