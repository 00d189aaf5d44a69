"""Options that left the library: "pipeline" 3 (hybrid: the first bounces per bounce, the deeper ones by the frame kernel),
its "hybrid_level", and "shade_pair" (the lighting of a bounce and the shading of the next in one launch).  Asking for one is
refused with NDT_E_INVALID and a text that names what was asked for, and a refusal leaves the context as it was: it renders
the bytes and counts it rendered before.

Needs a real MI355X: run with `pytest -m gpu`.
"""
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

NDT_E_INVALID = -1


def test_retired_options_are_refused_and_change_nothing():
    from ndt_amd.hip import NdtHip, NdtHipError
    g = golden("c3_random4d")
    gpu = NdtHip(0)
    try:
        gpu.upload_scene(g.scene)
        before, st0 = gpu.render(64, 36, 4)
        for name, value, text in (("pipeline", 3, "pipeline 3"), ("hybrid_level", 2, "hybrid_level"), ("shade_pair", 0, "shade_pair")):
            with pytest.raises(NdtHipError) as e:
                gpu.set_option(name, value)
            assert e.value.code == NDT_E_INVALID, name
            assert text in str(e.value), (name, str(e.value))
            assert text in (gpu.lib.ndt_hip_last_error() or b"").decode(), name
        after, st1 = gpu.render(64, 36, 4)
    finally:
        gpu.close()
    assert before.shape == after.shape and before.tobytes() == after.tobytes()
    for field in ("rays_primary", "rays_secondary", "rays_shadow", "rays_ref_equiv", "levels"):
        assert getattr(st0, field) == getattr(st1, field), field
    assert st0.rays_secondary > 0 and st0.rays_shadow > 0
