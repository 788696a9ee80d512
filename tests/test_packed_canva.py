"""The packed canva (rt.h "packed canva transport"): one 32-bit word per pixel,
f0 | f1 << 9 | f2 << 18, field = the channel's value for the integers 0..255
and 256 for everything else, which unpacks as -2147483648.0.

Without a GPU: the symbols, the host unpack against a NumPy restatement of
rt.h's text, what the entry points refuse before any device work, the flag of
rt_params.gather, the drop-ins' switch and the new kernels' resource usage.
On the GPU: the pack and unpack kernels against the same restatement.
Comparisons are bit for bit, on uint64 views.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import tipe_rt
from packed_canva_support import MARKER, every_value_plane, np_field, np_pack, np_unpack, same_bits
from tipe_rt import types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["rt_canva_pack_async", "rt_canva_unpack_async", "rt_canva_unpack_host", "rt_assemble_packed_async",
               "rt_set_fill_packed_canva"]


# ---- without a GPU ---------------------------------------------------------------

def test_symbols_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", tipe_rt.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [s for s in NEW_SYMBOLS if s not in syms]
    assert set(NEW_SYMBOLS) <= set(tipe_rt.EXPORTED_SYMBOLS)
    assert T.RT_GATHER_PACKED_CANVA == 0x100
    hdr = open(os.path.join(ROOT, "include", "rt", "rt.h")).read()
    assert re.search(r"#define\s+RT_GATHER_PACKED_CANVA\s+0x100\b", hdr)


def test_restatement_packs_the_marker_for_everything_else():
    odd = np.array([[np.nan, 0.5, 256.0], [-1.0, -0.0, np.inf], [255.0, 0.0, 1.0]])
    assert np_field(odd).tolist() == [[256, 256, 256], [256, 256, 256], [255, 0, 1]]
    assert int(np_pack(np.array([[3.0, MARKER, 255.0]]))[0]) == 3 | 256 << 9 | 255 << 18


def test_host_unpack_every_value_in_every_position():
    px = every_value_plane()
    words = np_pack(px)
    assert (words >> np.uint32(27) == 0).all()
    same_bits(np_unpack(words), px)                      # the restatement round-trips the 257 values
    got = tipe_rt.canva_unpack_host(words)
    same_bits(got, px)
    # bits 27..31 are ignored
    for high in (0xF8000000, 0x08000000, 0x80000000):
        same_bits(tipe_rt.canva_unpack_host(words | np.uint32(high)), px)
    # fields 257..511, which no pack writes, are the marker too
    same_bits(tipe_rt.canva_unpack_host(np.array([257 | 511 << 9 | 300 << 18], dtype=np.uint32)),
              np.full((1, 3), MARKER))
    # -0.0 never comes out: field 0 is +0.0
    assert not np.signbit(tipe_rt.canva_unpack_host(np.zeros(4, dtype=np.uint32))).any()


def test_refusals_before_any_device_work():
    L = tipe_rt.lib()
    words = (C.c_uint * 8)()
    cols = (C.c_double * 24)()
    w, c = C.addressof(words), C.addressof(cols)
    for fn, a, b in ((L.rt_canva_pack_async, c, w), (L.rt_canva_unpack_async, w, c)):
        assert fn(4, None, b, None) == T.RT_EINVAL
        assert fn(4, a, None, None) == T.RT_EINVAL
        assert fn(0, a, b, None) == T.RT_EINVAL
        assert fn(-3, a, b, None) == T.RT_EINVAL
        assert fn((1 << 30) + 1, a, b, None) == T.RT_EINVAL
        assert b"2^30" in L.rt_last_error()
    assert L.rt_canva_pack_async(4, c, w + 2, None) == T.RT_EINVAL
    assert b"aligned" in L.rt_last_error()
    assert L.rt_canva_unpack_async(4, w + 1, c, None) == T.RT_EINVAL
    assert L.rt_canva_unpack_host(4, None, c) == T.RT_EINVAL
    assert L.rt_canva_unpack_host(4, w, None) == T.RT_EINVAL
    assert L.rt_canva_unpack_host(0, w, c) == T.RT_EINVAL
    assert L.rt_canva_unpack_host((1 << 30) + 1, w, c) == T.RT_EINVAL
    assert L.rt_canva_unpack_host(4, w + 3, c) == T.RT_EINVAL
    assert L.rt_canva_unpack_host(4, w + 4, c) == T.RT_OK
    # rt_assemble_packed_async: rt_assemble_async's rules, and the alignment
    assert L.rt_assemble_packed_async(None, 0, 1, 1, 1, 1, 1, c, None) == T.RT_EINVAL
    assert L.rt_assemble_packed_async(w, 0, 1, 1, 1, 1, 1, None, None) == T.RT_EINVAL
    assert L.rt_assemble_packed_async(w + 2, 0, 1, 1, 1, 1, 1, c, None) == T.RT_EINVAL
    assert L.rt_assemble_packed_async(w, 0, 2, 4, 4, 10, 30, c, None) == T.RT_EINVAL      # 2 x 1 tiles < 8 tiles
    assert L.rt_assemble_packed_async(w, 0, 1, 2, 3, 1, 1, c, None) == T.RT_EINVAL        # rows not whole tiles
    assert L.rt_assemble_packed_async(w, 1, 1, 2, 2, 2, 2, c, None) == T.RT_EINVAL        # stride overlaps
    assert b"rank_stride" in L.rt_last_error()


def test_gather_flag_passes_params_validation():
    """rt_render_gather_async validates the params and then refuses
    tile_rows = 0, all before any device work: its error tells which check
    spoke."""
    L = tipe_rt.lib()
    sc = T.Scene()
    p = T.Params()
    L.rt_params_init(C.byref(p))
    assert p.gather == T.RT_GATHER_RCCL                       # the default is unchanged
    p.largeur_image, p.hauteur_image, p.nbRayonParPixel, p.nbRebondMax = 8, 6, 1, 5
    buf = (C.c_double * (8 * 6 * 3))()
    fr = T.Frame(C.addressof(buf), None, None, None)

    def refused_by_params(gather):
        p.gather = gather
        assert L.rt_render_gather_async(C.byref(sc), C.byref(p), 0, C.byref(fr), None) == T.RT_EINVAL
        return b"gather transport" in L.rt_last_error()

    for ok in (T.RT_GATHER_RCCL, T.RT_GATHER_PEER, T.RT_GATHER_RCCL | T.RT_GATHER_PACKED_CANVA,
               T.RT_GATHER_PEER | T.RT_GATHER_PACKED_CANVA):
        assert not refused_by_params(ok), ok                  # refused later: tile_rows 0
        assert b"tile_rows" in L.rt_last_error()
    for bad in (2, 0x200, 0x102, 0x300, -1, 7):
        assert refused_by_params(bad), bad


def test_fill_switch_returns_previous_setting():
    L = tipe_rt.lib()
    assert L.rt_set_fill_packed_canva(0) == 0                 # off by default
    try:
        assert L.rt_set_fill_packed_canva(1) == 0
        assert L.rt_set_fill_packed_canva(5) == 1             # any non-zero value is "on"
        assert L.rt_set_fill_packed_canva(0) == 1
        assert tipe_rt.set_fill_packed_canva(True) is False
        assert tipe_rt.set_fill_packed_canva(False) is True
    finally:
        L.rt_set_fill_packed_canva(0)


def test_new_kernels_use_no_scratch_and_no_lds():
    """The resource-usage target's line for rt_pack.hip (the Makefile's own
    flags): no scratch, no spills and no LDS for each of the three kernels."""
    mk = ["make", "-C", os.path.join(ROOT, "tipe-raytracer_amd")]
    lines = subprocess.run(mk + ["-n", "-B", "resource-usage"], capture_output=True, text=True, check=True).stdout
    cmd = [ln for ln in lines.splitlines() if "rt_pack.hip" in ln and "kernel-resource-usage" in ln]
    assert len(cmd) == 1, lines
    out = subprocess.run(cmd[0], shell=True, cwd=os.path.join(ROOT, "tipe-raytracer_amd"), capture_output=True,
                         text=True)
    txt = out.stdout + out.stderr
    assert out.returncode == 0, txt[-2000:]
    for name in ("canva_pack_kernel", "canva_unpack_kernel", "assemble_packed_kernel"):
        m = re.search(r"Function Name: \S*" + name + r"E.*?ScratchSize \[bytes/lane\]: (\d+).*?"
                      r"SGPRs Spill: (\d+).*?VGPRs Spill: (\d+).*?LDS Size \[bytes/block\]: (\d+)", txt, re.S)
        assert m, (name, txt[-2000:])
        assert [int(g) for g in m.groups()] == [0, 0, 0, 0], (name, m.groups())


# ---- on the GPU -------------------------------------------------------------------

def _pack_on_device(px, stream=None):
    import torch
    n = len(px)
    d = torch.from_numpy(np.ascontiguousarray(px)).to("cuda:0")
    words = torch.full((n + 2,), 0x7fffffff, dtype=torch.int32, device="cuda:0")     # guards around the n words
    back = torch.full((n + 2, 3), -5.0, dtype=torch.float64, device="cuda:0")
    st = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(st):
        tipe_rt.canva_pack_async(n, d.data_ptr(), words[1:].data_ptr(), st.cuda_stream)
        tipe_rt.canva_unpack_async(n, words[1:].data_ptr(), back[1:].data_ptr(), st.cuda_stream)
    st.synchronize()
    w = words.cpu().numpy().view(np.uint32)
    b = back.cpu().numpy()
    assert w[0] == 0x7fffffff and w[-1] == 0x7fffffff, "pack wrote outside its n words"
    assert (b[0] == -5.0).all() and (b[-1] == -5.0).all(), "unpack wrote outside its n colours"
    return w[1:-1], b[1:-1]


@pytest.mark.gpu
def test_device_pack_unpack_every_value():
    px = every_value_plane()
    words, back = _pack_on_device(px)
    assert (words == np_pack(px)).all()
    same_bits(back, px)
    same_bits(tipe_rt.canva_unpack_host(words), px)


@pytest.mark.gpu
def test_device_pack_values_outside_the_set_become_the_marker():
    odd = [np.nan, 0.5, 256.0, -1.0, -0.0]
    px = np.array([[v, 7.0, 255.0] for v in odd] + [[1.0, v, 0.0] for v in odd] + [[254.0, 2.0, v] for v in odd]
                  + [[np.nan, -0.0, 0.5], [np.inf, -np.inf, 1e300], [254.999, 1e-300, -2147483648.0]])
    words, back = _pack_on_device(px)
    assert (words == np_pack(px)).all()
    want = px.copy()
    want[np_field(px) == 256] = MARKER
    same_bits(back, want)
    assert (back[:5, 0] == MARKER).all() and (back[5:10, 1] == MARKER).all() and (back[10:15, 2] == MARKER).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 65])
def test_device_pack_small_counts(n):
    """One pixel, and one wave plus one lane."""
    px = every_value_plane()[300:300 + n]
    words, back = _pack_on_device(px)
    assert (words == np_pack(px)).all()
    same_bits(back, px)


@pytest.mark.gpu
def test_device_pack_on_a_side_stream():
    """More than one block (771 > 256), on a stream of the caller's: the two
    launches are ordered by that stream alone."""
    import torch
    px = every_value_plane()
    words, back = _pack_on_device(px, torch.cuda.Stream())
    assert (words == np_pack(px)).all()
    same_bits(back, px)
