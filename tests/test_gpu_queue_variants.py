"""Every render_kernel_q instantiation, once: six (QB, OPQ) values x sky
off/on x AO off/on = 24 kernels (rt_kernels.hip with_queue_variant).

The host maps (qb, opq, sky, ao) to the instantiation in one place; each
case here renders a scene that plan_render sends to one of them, checks
rt_last_render_kernel's name and compares all four planes with the oracle
bit for bit.  The sky halves use sky_scene()'s enclosing sky sphere (the
last sphere, main.c:64-71) and texels with sky_mode 1.
"""
import pytest

from gpu_driver import render_and_compare
from kernel_cases import VARIANTS, bundle_of, variant_params

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("ao", [False, True], ids=["noao", "ao"])
@pytest.mark.parametrize("sky", [False, True], ids=["nosky", "sky"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_queue_variant(variant, sky, ao):
    name, extra, mesh = VARIANTS[variant]
    bundle = bundle_of(extra, mesh(), sky)
    kernel = render_and_compare(bundle, variant_params(sky, ao))
    assert kernel == name
