"""What the tests of rt_set_accumulate_queue share: the switch as a context
manager that always restores 0, the scenes that reach each of the seven
(QB, OPQ) pairs of the task-queue kernel (kernel_cases.VARIANTS and the wide
tree of accumulate_support.SCENES) with their frames, and one upload of each."""
import contextlib

import helpers
import kernel_cases as kc
import tipe_rt
from accumulate_support import SCENES

# pair -> (render_kernel_q's name, builder(sky) of the bundle)
PAIRS = {key: (name, (lambda sky, extra=extra, mesh=mesh: kc.bundle_of(extra, mesh(), sky)))
         for key, (name, extra, mesh) in kc.VARIANTS.items()}
PAIRS["QB5"] = (kc.QB5, lambda sky: SCENES["wide_sky" if sky else "wide"][0]())
# the sphere pair and the tree pair that also run with the sky and with AO
FEATURED = ("QB-2", "QB3OP")


def frame_of(pair):
    """(W, H, bounces): accumulate_support.WORD_FRAMES' shapes -- two blocks
    wide, no multiple of 16; the wide tree at test_gpu_big_mesh's scale."""
    return (16, 12, 2) if pair == "QB5" else (21, 13, 5)


def queue_name(pair):
    return PAIRS[pair][0]


def list_name(pair):
    return PAIRS[pair][0].replace("render_kernel_q<", "render_kernel_ql<")


def params_of(pair, S, sky=False, ao=False, chunks=1, H=None):
    W, H0, B = frame_of(pair)
    return helpers.params(W, H if H is not None else H0, S, B, use_ao=ao, ao=2.5, chunks=chunks,
                          sky_mode=1 if sky else 0)


@contextlib.contextmanager
def accumulate_queue(on=True):
    """The switch set for the block; 0, its default, afterwards."""
    tipe_rt.set_accumulate_queue(on)
    try:
        yield
    finally:
        tipe_rt.set_accumulate_queue(False)


class PairUploads:
    """(pair, sky) -> (bundle, device scene), each built and uploaded once, until release()."""

    def __init__(self):
        self.up = {}

    def __call__(self, pair, sky=False):
        if (pair, sky) not in self.up:
            bundle = PAIRS[pair][1](sky)
            self.up[(pair, sky)] = (bundle, tipe_rt.DeviceScene(bundle.scene, 0))
        return self.up[(pair, sky)]

    def release(self):
        while self.up:
            self.up.popitem()[1][1].close()
