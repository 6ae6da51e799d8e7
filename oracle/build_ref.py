"""Recipe for oracle/_ref/libstm_ref_hip.so: the reference project's own kernels, translated by hipify-perl and compiled
for gfx950, so that the GPU tests can run them next to the oracle and the HIP library (tests/test_gpu_reference.py).

Nothing of the reference is kept in this repository: its *.cu / *.h are copied to a temporary directory outside the
tree, translated and compiled there, and only the linked library lands in oracle/_ref/ (git-ignored).  What is committed
is this script, four EMPTY stand-ins for the OpenCV headers that d_io.h includes (d_io.cu uses nothing from OpenCV) and
ref_recipe/inert_texture.h for the one dead texture entry point of the bilateral file.

Flags:  -fgpu-rdc      alu_hamdist_64 and alu_bilinear_interp* are __device__ functions called across files.
        -ffp-contract=off   SURVEY A-Q4 defines the oracle without contraction; what nvcc contracted in the original
                       build is unknowable, so the reference is compiled under the oracle's rule.
        -Wl,-Bsymbolic the product library's drop-in layer exports the same 33 mangled names; the reference library
                       must bind its own calls to its own definitions when both are loaded.
Left out: d_tx_scale_tex.cu, a dead texture entry point outside the reference's own makefile.

    python oracle/build_ref.py [REFERENCE_DIR]     (default: $STM_REFERENCE_DIR, else /root/reference)

With no reference tree the script does nothing and keeps whatever oracle/_ref/ holds."""
import concurrent.futures
import glob
import hashlib
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
RECIPE = os.path.join(HERE, "ref_recipe")
OUT_DIR = os.path.join(HERE, "_ref")
LIB = os.path.join(OUT_DIR, "libstm_ref_hip.so")
STAMP = os.path.join(OUT_DIR, "stamp.sha256")
SKIP = {"d_tx_scale_tex.cu"}
FLAGS = ["-O2", "-fPIC", "-fgpu-rdc", "--offload-arch=gfx950", "-ffp-contract=off", "-w"]
MAX_JOBS = 16


def _rocm_bin():
    for root in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if root and os.path.exists(os.path.join(root, "bin", "hipify-perl")):
            return os.path.join(root, "bin")
    exe = shutil.which("hipify-perl")
    return os.path.dirname(exe) if exe else None


def _recipe_files():
    out = [os.path.abspath(__file__)]
    for d, _, fs in os.walk(RECIPE):
        out += [os.path.join(d, f) for f in fs]
    return sorted(out)


def _stamp(ref_dir):
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(ref_dir, "*.cu")) + glob.glob(os.path.join(ref_dir, "*.h"))) + _recipe_files():
        h.update(os.path.basename(f).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(hashlib.sha256(fh.read()).digest())
    return h.hexdigest()


def build(ref_dir=None, verbose=False):
    """Returns the library's path, or None if there is neither a reference tree nor an earlier build."""
    ref_dir = ref_dir or os.environ.get("STM_REFERENCE_DIR") or "/root/reference"
    if not glob.glob(os.path.join(ref_dir, "d_*.cu")):
        return LIB if os.path.exists(LIB) else None
    stamp = _stamp(ref_dir)
    if os.path.exists(LIB) and os.path.exists(STAMP) and open(STAMP).read().strip() == stamp:
        return LIB
    rocm = _rocm_bin()
    assert rocm, "hipify-perl not found (ROCM_PATH)"
    hipcc, hipify = os.path.join(rocm, "hipcc"), os.path.join(rocm, "hipify-perl")
    tmp = tempfile.mkdtemp(prefix="stm_ref_build_")
    assert not os.path.realpath(tmp).startswith(os.path.realpath(os.path.dirname(HERE)) + os.sep)
    try:
        units = []
        for f in sorted(glob.glob(os.path.join(ref_dir, "*.cu")) + glob.glob(os.path.join(ref_dir, "*.h"))):
            name = os.path.basename(f)
            if name in SKIP:
                continue
            with open(os.path.join(tmp, name), "w") as out:
                subprocess.check_call([hipify, f], stdout=out, stderr=subprocess.DEVNULL)
            if name.endswith(".cu"):
                units.append(name)

        def compile_one(name):
            cmd = [hipcc, "-x", "hip"] + FLAGS + ["-I", tmp, "-I", os.path.join(RECIPE, "stubs")]
            if name == "d_filter_bilateral.cu":
                cmd += ["-include", os.path.join(RECIPE, "inert_texture.h")]
            obj = name[:-3] + ".o"
            subprocess.check_call(cmd + ["-c", name, "-o", obj], cwd=tmp)
            if verbose:
                print("  compiled", name, flush=True)
            return obj

        with concurrent.futures.ThreadPoolExecutor(max_workers=min(MAX_JOBS, len(units))) as ex:
            objs = list(ex.map(compile_one, units))
        os.makedirs(OUT_DIR, exist_ok=True)
        part = os.path.join(tmp, "libstm_ref_hip.so")
        subprocess.check_call([hipcc, "-fgpu-rdc", "--hip-link", "--offload-arch=gfx950", "-shared", "-Wl,-Bsymbolic",
                               "-o", part] + objs, cwd=tmp)
        shutil.copyfile(part, LIB)
        with open(STAMP, "w") as fh:
            fh.write(stamp + "\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return LIB


if __name__ == "__main__":
    print(build(sys.argv[1] if len(sys.argv) > 1 else None, verbose=True))
