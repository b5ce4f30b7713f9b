"""Static instruction mix of the banked kernels compiled per mechanism (csrc/rbd_jit.hip spec_bank_source), without a GPU: the program the
library generates for Atlas (floating base) is cross-compiled for gfx950 against the headers of a git revision (the parent) and against those of the working tree,
and the instructions of each kernel are counted per class, with its registers, scratch and LDS.  One wavefront per SIMD runs this code, so every instruction that
is not arithmetic is issue time (DESIGN.md §3.2's table prices the classes).

After the mix, the waits (a report): for every s_waitcnt that waits for a load its distance, in instructions, from the last load it covers, and how many of
them follow their load closely (kernel_waits).

usage: python scripts/bank_isa_mix.py [--parent REV] [--variant NAME:-DX=0[,-DY=0]] ... [--kernels aba_bank_spec,...] > profiles/bank_diet_isa.txt
  --parent REV    the revision whose headers make the first column (default HEAD; "none": no parent column)
  --variant ...   further columns: the working tree's headers with the given definitions (a part switched off: -DRBD_BANK_COMMIT_INPLACE=0)
The program text is the one the built library generates (rbd_amd.jit_source); the headers alone differ between the columns."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# what hiprtc gets (rbd_jit.hip kBaseOptions)
BASE_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast", "-DRBD_JIT_COMPILE"]
CLASSES = ("fp arithmetic", "DPP moves", "64-bit moves", "other vector", "scalar", "LDS", "global")
DETAIL = ("s_and_saveexec", "s_cbranch", "s_waitcnt", "s_nop", "s_mov", "v_mov_b32_e", "v_cndmask", "v_mul_lo_u32", "v_mad_u64_u32")
_FP = re.compile(r"^v_(pk_)?(fmac|fma|add|sub|mul|mad|mac|rcp|rsq|sqrt|div_scale|div_fmas|div_fixup|fract|floor|trunc|rndne|ldexp|min|max|frexp_mant)_f(16|32|64)(_e32|_e64|_sdwa)?$")


def classify(mnemonic, operands):
    if mnemonic.startswith("v_"):
        if "_dpp" in mnemonic or re.search(r"\b(row_sh[lr]|wave_sh[lr]|quad_perm|row_bcast|row_mirror|row_ror|wave_ro[lr])\b", operands):
            return "DPP moves"
        if mnemonic.startswith("v_mov_b64"):
            return "64-bit moves"
        return "fp arithmetic" if _FP.match(mnemonic) else "other vector"
    if mnemonic.startswith("s_"):
        return "scalar"
    if mnemonic.startswith("ds_"):
        return "LDS"
    if mnemonic.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "global"
    return None


def kernel_mix(asm_text, kernel):
    """counts per class (and per DETAIL mnemonic prefix) of the instructions between `kernel:` and its .Lfunc_end"""
    m = re.search(r"^%s:[^\n]*$(.*?)^\.Lfunc_end\d+:" % re.escape(kernel), asm_text, re.M | re.S)
    if m is None:
        raise KeyError(kernel)
    mix = dict.fromkeys(CLASSES + DETAIL, 0)
    for line in m.group(1).splitlines():
        line = line.split(";")[0].strip()
        if not line or line.endswith(":") or line.startswith("."):
            continue
        parts = line.split(None, 1)
        cls = classify(parts[0], parts[1] if len(parts) > 1 else "")
        if cls is None:
            continue
        mix[cls] += 1
        for d in DETAIL:
            if parts[0].startswith(d):
                mix[d] += 1
    return mix


def kernel_body(asm_text, kernel):
    """(mnemonic, operands) of the instructions between `kernel:` and its .Lfunc_end, in program order"""
    m = re.search(r"^%s:[^\n]*$(.*?)^\.Lfunc_end\d+:" % re.escape(kernel), asm_text, re.M | re.S)
    if m is None:
        raise KeyError(kernel)
    out = []
    for line in m.group(1).splitlines():
        line = line.split(";")[0].strip()
        if not line or line.endswith(":") or line.startswith("."):
            continue
        parts = line.split(None, 1)
        if classify(parts[0], parts[1] if len(parts) > 1 else "") is not None:
            out.append((parts[0], parts[1] if len(parts) > 1 else ""))
    return out


NEAR = {"global": 40, "LDS": 12}  # a wait this close behind the load it waits for leaves most of the round trip exposed (one wavefront per SIMD: nobody else issues)


def kernel_waits(asm_text, kernel):
    """For every s_waitcnt of `kernel` that waits for a load: (index of the wait, "global" | "LDS" | "scalar", distance in instructions from the LAST load it
    covers).  The counters are followed along the program text as if it were straight-line code (branches are not followed: the looped kernels would need that,
    the unrolled program's branches are short exec-mask skips): vmcnt counts global loads and stores, lgkmcnt LDS operations and scalar loads, both in issue
    order; `s_waitcnt vmcnt(N)` covers every operation but the N issued last.  A wait that covers no load that an earlier wait has not covered is left out."""
    queues = {"vm": [], "lgkm": []}  # outstanding operations: (index, kind)
    waits = []
    for i, (mn, ops) in enumerate(kernel_body(asm_text, kernel)):
        if mn.startswith(("global_load", "flat_load", "buffer_load")):
            queues["vm"].append((i, "global"))
        elif mn.startswith(("global_store", "flat_store", "buffer_store", "global_atomic")):
            queues["vm"].append((i, None))
        elif mn.startswith("ds_"):
            queues["lgkm"].append((i, "LDS" if mn.startswith(("ds_read", "ds_load", "ds_bpermute", "ds_permute", "ds_swizzle")) else None))
        elif mn.startswith(("s_load", "s_buffer_load")):
            queues["lgkm"].append((i, "scalar"))
        elif mn == "s_waitcnt":
            for q, name in (("vm", "vmcnt"), ("lgkm", "lgkmcnt")):
                c = re.search(name + r"\((\d+)\)", ops)
                if c is None:
                    continue
                n = int(c.group(1))
                covered = queues[q][:len(queues[q]) - n] if n else queues[q]
                queues[q] = queues[q][len(queues[q]) - n:] if n else []
                loads = [e for e in covered if e[1] is not None]
                if loads:
                    waits.append((i, loads[-1][1], i - loads[-1][0]))
    return waits


def kernel_resources(asm_text, kernel):
    """VGPRs, AGPRs, scratch bytes, LDS bytes, spilled VGPRs of `kernel` from the code object's metadata (amdhsa.kernels)"""
    for blk in re.split(r"^\s*- \.agpr_count:", asm_text, flags=re.M)[1:]:
        name = re.search(r"^\s*\.name:\s*(\S+)", blk, re.M)
        if name is None or name.group(1) != kernel:
            continue
        get = lambda key: int(re.search(r"^\s*\.%s:\s*(\d+)" % key, blk, re.M).group(1))
        return {"vgprs": get("vgpr_count"), "agprs": int(blk.split()[0]), "scratch": get("private_segment_fixed_size"), "lds": get("group_segment_fixed_size"),
                "vgpr_spills": get("vgpr_spill_count")}
    raise KeyError(kernel)


def compile_asm(source, csrc, include, defines=(), workdir=None):
    """device assembly (text) of `source` compiled the way rbd_jit.hip compiles it, against the headers in `csrc` and `include`"""
    d = workdir or tempfile.mkdtemp(prefix="rbd_isa_")
    try:
        src = os.path.join(d, "program.hip")
        with open(src, "w") as f:
            f.write(source)
        out = os.path.join(d, "program.s")
        subprocess.run([HIPCC] + BASE_FLAGS + list(defines) + ["-I", csrc, "-I", include, "--cuda-device-only", "-S", src, "-o", out], check=True, capture_output=True, text=True)
        return open(out).read()
    finally:
        if workdir is None:
            shutil.rmtree(d, ignore_errors=True)


def atlas_sources():
    import torch
    sys.path.insert(0, ROOT)
    import rbd_amd as rbd
    model = rbd.load_flat_model(os.path.join(ROOT, "tests", "golden", "models", "atlas_floating.json"))
    return {"f64": rbd.jit_source(model, torch.float64, "banked"), "f32": rbd.jit_source(model, torch.float32, "banked")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="HEAD")
    ap.add_argument("--variant", action="append", default=[])
    ap.add_argument("--kernels", default="aba_bank_spec,aba_bank_fused_spec,rnea_bank_spec")
    a = ap.parse_args()
    sources = atlas_sources()
    columns = []  # (title, csrc, include, defines)
    tmp = None
    if a.parent != "none":
        tmp = tempfile.mkdtemp(prefix="rbd_isa_parent_")
        tar = subprocess.run(["git", "-C", ROOT, "archive", a.parent, "rigidbodydynamics.jl_amd/csrc", "include"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", a.parent], check=True, capture_output=True, text=True).stdout.strip()
        columns.append(("parent " + rev, os.path.join(tmp, "rigidbodydynamics.jl_amd", "csrc"), os.path.join(tmp, "include"), ()))
    here = (os.path.join(ROOT, "rigidbodydynamics.jl_amd", "csrc"), os.path.join(ROOT, "include"))
    columns.append(("branch", here[0], here[1], ()))
    for v in a.variant:
        name, _, defs = v.partition(":")
        columns.append((name, here[0], here[1], tuple(defs.split(","))))
    try:
        for sfx, source in sources.items():
            with ThreadPoolExecutor(max(1, min(len(columns), len(os.sched_getaffinity(0))))) as pool:
                asms = list(pool.map(lambda c: compile_asm(source, c[1], c[2], c[3]), columns))
            for k in a.kernels.split(","):
                kernel = "%s_%s" % (k, sfx)
                print("== %s (Atlas, floating base) ==" % kernel)
                print("%-16s" % "" + "".join("%22s" % c[0][:21] for c in columns))
                mixes = [kernel_mix(s, kernel) for s in asms]
                res = [kernel_resources(s, kernel) for s in asms]
                for row in CLASSES:
                    print("%-16s" % row + "".join("%22d" % m[row] for m in mixes))
                print("%-16s" % "all" + "".join("%22d" % sum(m[c] for c in CLASSES) for m in mixes))
                for row in DETAIL:
                    print("%-16s" % ("  " + row + "*") + "".join("%22d" % m[row] for m in mixes))
                waits = [kernel_waits(s, kernel) for s in asms]
                for kind in ("global", "LDS"):
                    print("%-16s" % ("waits: " + kind) + "".join("%22d" % sum(1 for w in ws if w[1] == kind) for ws in waits))
                    print("%-16s" % ("  within %d" % NEAR[kind]) + "".join("%22d" % sum(1 for w in ws if w[1] == kind and w[2] <= NEAR[kind]) for ws in waits))
                for row, key in (("VGPRs", "vgprs"), ("AGPRs", "agprs"), ("scratch bytes", "scratch"), ("spilled VGPRs", "vgpr_spills"), ("LDS bytes", "lds")):
                    print("%-16s" % row + "".join("%22d" % r[key] for r in res))
                # every wait: instruction index of the s_waitcnt : distance from the last load it covers (g global, l LDS, s scalar)
                for c, ws in zip(columns, waits):
                    print("waits of %s: " % c[0] + " ".join("%d:%s%d" % (w[0], w[1][0].lower(), w[2]) for w in ws))
                print()
    finally:
        if tmp:
            shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
