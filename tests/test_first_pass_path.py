"""Which kernel runs the frame's first horizontal pass, pinned through stm_first_pass_path (include/stm_hip.h): 0 where stm_k_pq_hc
(or another kernel) runs it, else the blocks per image row of stm_k_pq_hc2, which sweeps both views from one ring of costs.  Host
arithmetic only -- nothing is launched, no GPU is needed.

The expected values follow from the dispatcher (stm_kernels_aggm.hip: hc2_parts).  stm_k_pq_hc2 takes the frames that
stm_k_pq_hc<12, true> took: the PX fast path (48 < D <= 64, usd <= 36, no 0x100 / 0x200) where hc_waves says 12, which at D = 64 and
usd 34 is 18 <= zd <= 45 (tests/test_agg_path.py).  A row of at least eight 96-pixel segments is split into 2 row_split(W / 192)
parts unless the frame has 4096 rows or more.  stm_set_agg_variant(2000000) turns the kernel off, and stm_agg_path answers the same
under both."""
import pytest

SEPARATE_VIEWS = 2000000  # stm_k_pq_hc, one view per block
MP, PX, VREGS, HREGS = 1, 2, 4, 8


@pytest.fixture
def both(stm):
    """(first_pass_path, agg_path) of the arguments under the default variant, after asserting that under SEPARATE_VIEWS the
    first is 0 and the second unchanged"""
    from stm_amd import device_api as dev
    lib = stm.lib()

    def ask(*a):
        fp, ap = dev.first_pass_path(*a), dev.agg_path(*a)
        lib.stm_set_agg_variant(SEPARATE_VIEWS)
        try:
            fp_off, ap_off = dev.first_pass_path(*a), dev.agg_path(*a)
        finally:
            lib.stm_set_agg_variant(0)
        assert fp_off == 0 and ap_off == ap, (fp_off, hex(ap_off), hex(ap))
        return fp, ap
    return ask


def test_the_benchmark_frame(both):
    """1080 x 1920, D 64, zd 32, usd 34, stages 3: two parts per row, 2160 blocks as stm_k_pq_hc had; stm_agg_path as it was"""
    fp, ap = both(64, 32, 1080, 1920, 34, 3)
    assert fp == 2
    assert ap == MP | PX | VREGS | HREGS | (12 << 8)


@pytest.mark.parametrize("zd, parts", [(17, 0), (18, 1), (45, 1), (46, 0)])
def test_zero_disp(both, zd, parts):
    """outside 18..45 the 8-wave stm_k_pq_hc runs"""
    fp, ap = both(64, zd, 37, 67, 34, 3)
    assert fp == parts and ap & PX and (ap >> 8) & 0xff == (12 if parts else 8), (fp, hex(ap))


@pytest.mark.parametrize("D, parts", [(48, 0), (49, 1), (64, 1), (65, 0)])
def test_num_disp(both, D, parts):
    fp, ap = both(D, D // 2, 37, 67, 34, 3)
    assert fp == parts and bool(ap & PX) == bool(parts), (fp, hex(ap))


@pytest.mark.parametrize("usd, parts", [(29, 1), (36, 1), (37, 0)])
def test_usd(both, usd, parts):
    fp, ap = both(64, 32, 70, 40, usd, 3)
    assert fp == parts and bool(ap & PX) == bool(parts), (fp, hex(ap))


@pytest.mark.parametrize("stages, parts", [(1, 1), (3, 1), (3 | 0x100, 0), (3 | 0x200, 0), (3 | 0x400, 1)])
def test_stage_bits(both, stages, parts):
    """0x100 and 0x200 read a volume after the aggregation: the PQ layout, stm_k_pq_hc"""
    fp, ap = both(64, 32, 40, 72, 34, stages)
    assert fp == parts and bool(ap & PX) == bool(parts), (fp, hex(ap))


@pytest.mark.parametrize("H, W, parts", [(2, 672, 1), (2, 673, 2), (2, 700, 2), (4095, 1920, 2), (4096, 1920, 1), (2160, 3840, 2),
                                         (3, 4609, 4), (3, 7680, 6)])
def test_parts(both, H, W, parts):
    """eight segments (W > 672) are the first to be split; 4609 and 7680 columns are 25 and 40 segments of stm_k_pq_hc: row_split 2, 3"""
    fp, _ = both(64, 32, H, W, 34, 3)
    assert fp == parts


@pytest.mark.parametrize("variant", [1000000, 1000, 10000, 20000000, 100000000])
def test_other_variants_off_the_fast_path(stm, variant):
    """whatever takes the frame off stm_k_pq_hc<12, true> takes it off stm_k_pq_hc2"""
    from stm_amd import device_api as dev
    lib = stm.lib()
    lib.stm_set_agg_variant(variant)
    try:
        assert dev.first_pass_path(64, 32, 1080, 1920, 34, 3) == 0
    finally:
        lib.stm_set_agg_variant(0)
    assert dev.first_pass_path(64, 32, 1080, 1920, 34, 3) == 2


def test_arguments_no_frame_takes(both):
    assert both(0, 0, 10, 10, 34, 3) == (0, 0) and both(64, 32, 0, 10, 34, 3) == (0, 0) and both(64, 32, 10, 10, 0, 3) == (0, 0)
