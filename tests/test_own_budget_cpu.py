"""Register budgets of the owned spread kernels (the default bench line's kernel and cfg 3's), from
the gfx950 code objects hipRTC builds on a CPU host: at most 128 VGPRs at 4 waves per SIMD, no
scratch, no VGPR spill, and fewer SGPR spills than the 68 the classifier's kernel had before its
packet chain was reordered.  Built with that change: classifier 112 VGPRs and 62 SGPR
spills, parse5 126 VGPRs and 58."""
import pytest

from mimic_amd import jit, workloads as W


@pytest.mark.parametrize("prog", ["prog_classifier", "prog_parse5"])
def test_owned_kernel_register_budget(prog):
    p = getattr(W, prog)()
    src = jit.kernel_source([p.raw], 0, (), jit.spread_spec([(p.raw, p.relocs)], p.maps, 262144, own=True))
    r = jit.kernel_resources(jit.code_object(src))
    print(prog, r)
    assert r["vgpr_total"] <= 128 and r["waves_per_simd"] == 4
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0
    assert r["sgpr_spill"] < 68
