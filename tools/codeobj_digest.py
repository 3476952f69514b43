"""Digests of the gfx950 code objects of two builds of raytracer-server_amd, section by section.

python tools/codeobj_digest.py PARENT_TREE BRANCH_TREE [--out LOG]

Each tree is a checkout in which `make`, `make qcheck`, `make walkref`, `make near64`, `make ab` and `make dbg` ran
from raytracer-server_amd/ (build/, build_qcheck/, ... hold the kernel objects). For every kernel object of every
build the gfx950 code object is taken out of the offload bundle (the object's .hip_fatbin section,
clang-offload-bundler --unbundle) and its .text,
.rodata and .note sections (llvm-objcopy --only-section; .note holds the kernel metadata: registers, spills, LDS,
scratch, kernarg size) are hashed. The sections are compared, not the files: two compiles of one source from different
directories give the same sections in ELF files that differ elsewhere. Prints one line per (build, unit, section) with
both digests and `same` / `DIFFERENT`; exit status 1 if any section differs or is missing. Compares bytes only."""
import hashlib
import os
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
BUILDS = (("default", "build"), ("qcheck", "build_qcheck"), ("walkref", "build_walkref"), ("near64", "build_near64"),
          ("ab", "build_ab"), ("dbg", "build_dbg"))
UNITS = ("render_f64", "render_mesh_f64", "render_flat_f64", "wavefront_f64", "render_f32", "denoise", "accum",
         "reproject")
SECTIONS = (".text", ".rodata", ".note")


def section_digests(obj, tmp):
    """{section: (sha256 hex, size)} of the gfx950 code object bundled in `obj`."""
    fat, elf = os.path.join(tmp, "k.fatbin"), os.path.join(tmp, "k.elf")
    # the host object carries the offload bundle in its .hip_fatbin section
    subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj, os.path.join(tmp, "host.o")],
                   check=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={elf}"], check=True)
    out = {}
    for sec in SECTIONS:
        raw = os.path.join(tmp, "sec.bin")
        if os.path.exists(raw):
            os.remove(raw)
        subprocess.run([f"{LLVM}/llvm-objcopy", "-O", "binary", f"--only-section={sec}", elf, raw], check=True)
        data = open(raw, "rb").read() if os.path.exists(raw) else b""
        out[sec] = (hashlib.sha256(data).hexdigest(), len(data))
    return out


def main(argv):
    if len(argv) < 3:
        print(__doc__)
        return 2
    parent, branch = argv[1], argv[2]
    out = open(argv[argv.index("--out") + 1], "w") if "--out" in argv else None

    def emit(line):
        print(line)
        if out:
            out.write(line + "\n")

    bad = 0
    emit("# build unit section bytes parent_sha256 branch_sha256 verdict")
    with tempfile.TemporaryDirectory(prefix="codeobj_") as tmp:
        for name, bdir in BUILDS:
            for unit in UNITS:
                objs = [os.path.join(t, "raytracer-server_amd", bdir, "kernels", unit + ".o") for t in (parent, branch)]
                if not all(os.path.exists(o) for o in objs):
                    emit(f"{name} {unit} - - - - MISSING")
                    bad += 1
                    continue
                dp, db = section_digests(objs[0], tmp), section_digests(objs[1], tmp)
                for sec in SECTIONS:
                    same = dp[sec] == db[sec]
                    bad += not same
                    emit(f"{name} {unit} {sec} {dp[sec][1]}/{db[sec][1]} {dp[sec][0][:16]} {db[sec][0][:16]} "
                         f"{'same' if same else 'DIFFERENT'}")
    emit(f"# {len(BUILDS) * len(UNITS) * len(SECTIONS)} sections compared, {bad} different or missing")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
