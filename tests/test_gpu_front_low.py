"""The reduced-resolution frame's front as a stage on the GPU (stm_d_demux_sbs_low, stm_d_demux_nv12_low: the kernel
stm_k_front_low, and under stm_set_agg_variant(600) the chain of kernels it replaces), bit for bit against
test_reduced_stream_ref.reduced_front_ref: the split images, the reduced images and the census words of the reduced pair."""
import ctypes as C

import numpy as np
import pytest

from test_nv12_ref import nv12_to_bgr_ref, random_planes
from test_reduced_stream_ref import reduced_front_of_views, reduced_front_ref

pytestmark = pytest.mark.gpu

# (H, W, h, w): ratio 2 in one tile; a non-integer ratio; two tiles across and three down, ragged both ways; ratio 1; up-scaling;
# an image narrower than the census halo; one pixel
SHAPES = [(40, 64, 20, 32), (45, 77, 19, 35), (70, 150, 33, 70), (24, 40, 24, 40), (12, 20, 18, 30), (32, 48, 3, 5), (9, 9, 1, 1)]
SHAPE_IDS = ["%dx%d_to_%dx%d" % s for s in SHAPES]
SENTINEL = 0x5A


def seam_frame(seed, H, W, elem_sz, extra_cols=0):
    """a random side-by-side frame whose left eye ends in bright columns and whose right eye begins with dark ones (a tap or a
    halo pixel that crossed the half would show); extra_cols columns of SENTINEL follow the right eye"""
    rng = np.random.RandomState(seed)
    sbs = rng.randint(0, 256, size=(H, 2 * W + extra_cols, elem_sz)).astype(np.uint8)
    k = min(6, W)
    sbs[:, W - k:W, :3] = rng.randint(240, 256, size=(H, k, 3))
    sbs[:, W:W + k, :3] = rng.randint(0, 16, size=(H, k, 3))
    sbs[:, 2 * W:] = SENTINEL
    return sbs


def run_stage(stm, sbs, W, h, w, census, variant):
    """stm_d_demux_sbs_low on output buffers carved at odd addresses (the census planes at 4-byte-only aligned ones) from one
    arena whose margins must stay untouched.  Returns the six arrays (census None, None when not asked for) as they lie in memory:
    what the call did not write holds FILL."""
    import torch
    from test_gpu_caller_buffers import Arena, P, read
    lib = stm.lib()
    lib.stm_set_stream(C.c_void_p(torch.cuda.current_stream().cuda_stream))
    H, Wsbs, E = sbs.shape
    arena = Arena(True, nbytes=1 << 20)
    d_sbs = arena.put(sbs, 7)
    il, ir = arena.carve(H * W * E, 1), arena.carve(H * W * E, 11)
    ll, lr = arena.carve(h * w * E, 5), arena.carve(h * w * E, 13)
    cl, cr = (arena.carve(h * w * 4, 4), arena.carve(h * w * 4, 12)) if census else (None, None)
    lib.stm_set_agg_variant(variant)
    try:
        lib.stm_d_demux_sbs_low(P(il), P(ir), P(ll), P(lr), P(cl) if census else None, P(cr) if census else None, P(d_sbs), H, Wsbs, W, h, w, E)
        assert arena.intact()
    finally:
        lib.stm_set_agg_variant(0)
    assert np.array_equal(read(d_sbs, np.uint8, sbs.shape), sbs)  # the frame is read only
    return (read(il, np.uint8, (H, W, E)), read(ir, np.uint8, (H, W, E)), read(ll, np.uint8, (h, w, E)), read(lr, np.uint8, (h, w, E)),
            read(cl, np.uint32, (h, w)) if census else None, read(cr, np.uint32, (h, w)) if census else None)


def check(got, want, census):
    from test_gpu_caller_buffers import FILL
    for k in range(4):
        assert np.array_equal(got[k][..., :3], want[k][..., :3]), k
        assert (got[k][..., 3:] == FILL).all(), k  # bytes past a pixel's third are not written
    if census:
        assert np.array_equal(got[4], want[4]) and np.array_equal(got[5], want[5])


@pytest.mark.parametrize("elem_sz", [3, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_front_low_against_the_composition(gpu_ready, orc, stm, shape, elem_sz):
    """the fused kernel and the chain (variant 600), with and without census planes"""
    H, W, h, w = shape
    sbs = seam_frame(H * 3 + w + elem_sz, H, W, elem_sz)
    want = reduced_front_ref(orc, sbs, W, h, w)
    for variant in (0, 600):
        for census in (True, False):
            check(run_stage(stm, sbs, W, h, w, census, variant), want, census)


@pytest.mark.parametrize("elem_sz", [3, 4])
def test_front_low_wider_frame_never_shows_the_spare_columns(gpu_ready, orc, stm, elem_sz):
    H, W, h, w = SHAPES[1]
    sbs = seam_frame(91, H, W, elem_sz, extra_cols=5)
    want = reduced_front_ref(orc, np.ascontiguousarray(sbs[:, :2 * W]), W, h, w)
    got = run_stage(stm, sbs, W, h, w, True, 0)
    check(got, want, True)
    assert np.array_equal(got[3], run_stage(stm, sbs, W, h, w, True, 600)[3])


def test_front_low_narrow_frame_takes_the_chain(gpu_ready, orc, stm):
    """num_cols_sbs < 2 * num_cols: the plain split leaves the right image's last columns as they were (here the arena's fill),
    and the rest follows from the images as they then lie in memory"""
    from test_gpu_caller_buffers import FILL
    H, W, h, w = SHAPES[1]
    sbs = np.ascontiguousarray(seam_frame(92, H, W, 3)[:, :2 * W - 9])
    L, R = orc.demux_sbs(sbs, W)
    R[:, W - 9:] = FILL
    want = (L, R) + reduced_front_of_views(orc, L, R, h, w)
    check(run_stage(stm, sbs, W, h, w, True, 0), want, True)


NV12_CASES = [(40, 64, 20, 32, 6, 10), (46, 78, 19, 35, 3, 8)]  # (H, W, h, w, pitch_y - Wsbs, pitch_uv - Wsbs)


@pytest.mark.parametrize("matrix", [0, 1, 2, 3])
@pytest.mark.parametrize("case", NV12_CASES, ids=["40x64", "46x78"])
def test_front_low_nv12(gpu_ready, orc, stm, case, matrix):
    """stm_d_demux_nv12_low on pitched planes: the converted split images, their reduction and its census words; fused and chain"""
    import torch
    from stm_amd import device_api as dev
    H, W, h, w, dy, duv = case
    Wsbs = 2 * W
    y, uv = random_planes(H + matrix, H, Wsbs, Wsbs + dy, Wsbs + duv)
    want = reduced_front_ref(orc, nv12_to_bgr_ref(y, uv, matrix), W, h, w)
    d_y, d_uv = torch.from_numpy(np.array(y.base)).cuda()[:, :Wsbs], torch.from_numpy(np.array(uv.base)).cuda()[:, :Wsbs]
    lib = stm.lib()
    for variant in (0, 600):
        for elem_sz in (3, 4):
            il, ir = (torch.full((H, W, elem_sz), 9, dtype=torch.uint8, device="cuda") for _ in range(2))
            ll, lr = (torch.full((h, w, elem_sz), 9, dtype=torch.uint8, device="cuda") for _ in range(2))
            cl, cr = (torch.zeros((h, w), dtype=torch.int32, device="cuda") for _ in range(2))
            lib.stm_set_agg_variant(variant)
            try:
                dev.d_demux_nv12_low(il, ir, ll, lr, d_y, d_uv, matrix, cl, cr)
                torch.cuda.synchronize()
            finally:
                lib.stm_set_agg_variant(0)
            for g, wnt in zip((il, ir, ll, lr), want[:4]):
                g = g.cpu().numpy()
                assert np.array_equal(g[..., :3], wnt) and (g[..., 3:] == 9).all()
            assert np.array_equal(cl.cpu().numpy().view(np.uint32), want[4]) and np.array_equal(cr.cpu().numpy().view(np.uint32), want[5])


def test_host_flavour(gpu_ready, orc, stm):
    """stm_demux_sbs_low on host arrays; bytes past a pixel's third come back 0"""
    from stm_amd import host_api
    H, W, h, w = SHAPES[2]
    sbs = seam_frame(17, H, W, 4)
    want = reduced_front_ref(orc, sbs, W, h, w)
    got = host_api.demux_sbs_low(sbs, W, h, w)
    for g, wnt in zip(got, want):
        assert np.array_equal(g, wnt)
    assert host_api.demux_sbs_low(sbs, W, h, w, census=False)[4] is None
