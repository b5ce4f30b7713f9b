"""The host builds of the per-state routines under csrc/: a test hands over a C++ harness (extern "C" entry points around the RBD_HD routines it checks), build()
compiles it with ROCm's clang as plain C++ against the HIP shim header (tests/emu/spec_shim) and returns the loaded library.  The shared object is cached in the
temporary directory under a key of the harness text, EVERY header under csrc/ and the shim — a new or changed header can never leave a stale cache behind."""
import ctypes
import glob
import hashlib
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rigidbodydynamics.jl_amd", "csrc")
SHIM = os.path.join(ROOT, "tests", "emu", "spec_shim")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def build(harness_text, tag):
    """Compile `harness_text` (cached under <tmp>/<tag>/) and load it."""
    deps = sorted(glob.glob(os.path.join(CSRC, "*.hpp"))) + [os.path.join(SHIM, "hip", "hip_runtime.h")]
    key = hashlib.sha256((harness_text + "".join(open(f).read() for f in deps)).encode()).hexdigest()[:16]
    d = os.path.join(tempfile.gettempdir(), tag)
    os.makedirs(d, exist_ok=True)
    so = os.path.join(d, "emu_%s.so" % key)
    if not os.path.exists(so):
        src = os.path.join(d, "emu_%s.cpp" % key)
        open(src, "w").write(harness_text)
        subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=fast", "-Wno-everything",
                               "-I", SHIM, "-I", CSRC, "-I", os.path.join(ROOT, "include"), src, "-o", so + ".tmp"])
        os.replace(so + ".tmp", so)
    return ctypes.CDLL(so)
