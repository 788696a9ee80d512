"""The paired-draw form of render_kernel_q<QB=-2> (rt_queue.h, PD): every
material opaque and no AO, so bounce i of a sample takes draws 4 + 2i and
5 + 2i; a bounce with even i opens Philox block 1 + i/2 and keeps its words
2, 3 in registers for bounce i + 1.

24x18 pixels, 5 spp in 2 chunks: tasks of 2 and 3 samples, 864 tasks, four
waves, so a lane starts new samples and new tasks with the kept words of an
older sample still in place.  Bounce counts: 0 no cast at all, 1 no direction
is ever made, 2 one direction from a new block, 3 the first direction from kept
words, 6 the headline workload's, 7 a path ending on a half-used block.  All
four planes are compared with the oracle bit for bit.

The same frames through the general form: the alpha-0.5 sphere (QB -1, whose
refracting bounces take an odd number of draws) and AO on the plain box (the
AO kernel of QB -2, which keeps the block cache in LDS).

A camera inside the box that looks out of its open side: central pixels miss
at the first cast of every sample (resolve_hit's miss, whose two adds of
(0, 0, 0) the paired form does not make), outer pixels hit a wall sphere.
"""
import pytest

import helpers

from gpu_driver import render_and_compare
from kernel_cases import TRANSPARENT, bundle_of

pytestmark = pytest.mark.gpu

BOUNCES = [0, 1, 2, 3, 6, 7]
W, H, SPP, CHUNKS = 24, 18, 5, 2


@pytest.mark.parametrize("sky", [False, True], ids=["nosky", "sky"])
@pytest.mark.parametrize("bounces", BOUNCES)
def test_paired_draws_bounce_counts(bounces, sky):
    bundle = bundle_of((), None, sky)
    p = helpers.params(W, H, SPP, bounces, chunks=CHUNKS, sky_mode=1 if sky else 0)
    assert render_and_compare(bundle, p) == "render_kernel_q<QB=-2>"


@pytest.mark.parametrize("bounces", BOUNCES)
def test_general_draws_refraction(bounces):
    bundle = bundle_of(TRANSPARENT, None, False)
    p = helpers.params(W, H, SPP, bounces, chunks=CHUNKS)
    assert render_and_compare(bundle, p) == "render_kernel_q<QB=-1>"


@pytest.mark.parametrize("bounces", BOUNCES)
def test_general_draws_ao(bounces):
    bundle = bundle_of((), None, False)
    p = helpers.params(W, H, SPP, bounces, use_ao=True, ao=2.5, chunks=CHUNKS)
    assert render_and_compare(bundle, p) == "render_kernel_q<QB=-2>"


# Inside the box, looking out of its open side (+z).  The walls are spheres of
# radius 500 (x = 1 + z^2 / 1000 near the axis), so a ray leaves the box only
# within tan 0.063 of the axis: a 20 degree field (0.02 per pixel) puts a few
# central pixels wholly inside that cone and the outer ones on the walls.
OUTWARD_CAMERA = dict(origin=(0.0, 0.0, -1.0), target=(0.0, 0.0, 5.0), up=(0, 1, 0), vfov=20.0, ratio=4.0 / 3.0)


def test_paired_draws_misses():
    bundle = bundle_of((), None, False)
    p = helpers.params(W, H, SPP, 6, chunks=CHUNKS, cam=helpers.camera_of(OUTWARD_CAMERA))
    alb = helpers.oracle_render(bundle, p)["albedo"]
    zero = (alb == 0.0).all(axis=2)
    assert zero.any(), "no pixel misses on every sample"
    assert (~zero).any(), "no pixel hits"
    assert render_and_compare(bundle, p) == "render_kernel_q<QB=-2>"
