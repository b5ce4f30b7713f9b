"""Resources of the banked program compiled for Atlas (csrc/rbd_jit.hip spec_bank_source), cross-compiled for gfx950 without a device: one wavefront per SIMD runs
it, and scratch multiplies a lone wavefront's time, so every kernel of the program must keep all of its state in the 256 architectural VGPRs —
no scratch, no spills, no accumulation registers — and a workgroup's LDS must fit the CU's 160 KB.  The instruction mix itself is a report, not an assertion:
scripts/bank_isa_mix.py -> profiles/bank_diet_isa.txt."""
import importlib.util
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("aba_bank_spec", "aba_bank_fused_spec", "rnea_bank_spec")


def isa_mix():
    spec = importlib.util.spec_from_file_location("bank_isa_mix", os.path.join(ROOT, "scripts", "bank_isa_mix.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("dtype,sfx", [(torch.float64, "f64"), (torch.float32, "f32")])
def test_atlas_banked_program_resources(rbd, dtype, sfx):
    mix = isa_mix()
    if not os.path.exists(mix.HIPCC):
        pytest.skip("no hipcc to cross-compile with")
    model = rbd.load_flat_model(os.path.join(ROOT, "tests", "golden", "models", "atlas_floating.json"))
    source = rbd.jit_source(model, dtype, "banked")
    assert source is not None
    asm = mix.compile_asm(source, os.path.join(ROOT, "rigidbodydynamics.jl_amd", "csrc"), os.path.join(ROOT, "include"))
    for k in KERNELS:
        kernel = "%s_%s" % (k, sfx)
        res = mix.kernel_resources(asm, kernel)
        assert res["scratch"] == 0 and res["vgpr_spills"] == 0, (kernel, res)
        assert res["vgprs"] <= 256 and res["agprs"] == 0, (kernel, res)
        assert 0 < res["lds"] <= 160 * 1024, (kernel, res)
        counts = mix.kernel_mix(asm, kernel)
        # (the classifier sees the kernel: arithmetic dominates, the neighbour hops are DPP moves, nothing addresses scratch)
        assert counts["fp arithmetic"] > counts["scalar"] > 0 and counts["DPP moves"] > 0 and counts["LDS"] > 0, (kernel, counts)
