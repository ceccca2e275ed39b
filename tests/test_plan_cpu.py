"""CPU test of the per-chunk plan (plan_chunk, cylindertag_amd/csrc/ctag_api.hip): which kernel forms and grid sizes the library
picks for a chunk, from frame size, frame count, alignment, channels and the handle's options, with no developer aids set.
The expected values are the decisions the launchers made before the plan gathered them in one place."""
import pytest

import testkit as tk

# fields every chunk shares without developer aids
CONSTANT = dict(pack_max=8, pack_gx=32, scan_gx=48, mscan_gx=48, welsch_gs=1, welsch_gx=18, refine_gx=32, refine_sums_gx=12)
# a few frames (<= 4): latency-tuned kernels, every component a wave of its own
FEW = dict(latency=1, zero_first=0, mask_scan=0, prescan=0, all_wave=1, fork=0, big_points=1, big_cols=512, big_max_gx=8, refine="one")
# batches
MANY = dict(latency=0, zero_first=1, dec_zero_kernel=0, dec_zero_list=0, all_wave=0, fork=0, big_points=0x7fffffff, big_cols=4, big_max_gx=2)
FUSED_1080 = dict(fused=1, dec="mask", dec_xblocks=1, dec_yblocks=1, dec_band_rows=0, dec_bands=0, ccl="mask")

CASES = [
    # (id, chunk_plan arguments, expected fields)
    ("1080p_1", dict(rows=1080, cols=1920, nframes=1),
     dict(FEW, fused=0, dec_zero_kernel=0, dec_zero_list=1, dec="banded", dec_xblocks=2, dec_yblocks=32, dec_band_rows=5, ccl="tw5", small_cfg=1, refprm=1)),
    ("1080p_4", dict(rows=1080, cols=1920, nframes=4),
     dict(FEW, fused=0, dec_zero_kernel=0, dec_zero_list=1, dec="banded", dec_xblocks=2, dec_yblocks=32, dec_band_rows=5, ccl="tw5", small_cfg=1)),
    ("1080p_64", dict(rows=1080, cols=1920, nframes=64),
     dict(MANY, fused=0, dec="banded", dec_xblocks=2, dec_yblocks=4, dec_band_rows=34, ccl="tw5", small_cfg=1, mask_scan=0, prescan=0,
          refine="split_looping")),
    ("1080p_1024", dict(rows=1080, cols=1920, nframes=1024),
     dict(MANY, **FUSED_1080, small_cfg=1, mask_scan=1, prescan=1, refprm=1, refine="split_looping")),
    ("4k_256", dict(rows=2160, cols=3840, nframes=256),
     dict(MANY, fused=1, dec="mask", dec_xblocks=2, dec_yblocks=2, dec_bands=0, ccl="mask", small_cfg=0, mask_scan=1, prescan=1, refine="split_large")),
    ("1920x1200_1024", dict(rows=1200, cols=1920, nframes=1024),
     dict(MANY, fused=1, dec="mask_bands", dec_xblocks=1, dec_yblocks=1, dec_bands=4, ccl="mask", small_cfg=1, mask_scan=1, prescan=1,
          refine="split_looping")),
    ("640x480_1024", dict(rows=480, cols=640, nframes=1024),
     dict(MANY, fused=1, dec="mask_bands", dec_xblocks=1, dec_yblocks=1, dec_bands=4, ccl="mask", small_cfg=1, mask_scan=1, prescan=1)),
    ("640x480_64", dict(rows=480, cols=640, nframes=64),
     dict(MANY, fused=0, dec="banded", dec_xblocks=1, dec_yblocks=8, dec_band_rows=8, ccl="tw5", small_cfg=1, mask_scan=0, prescan=0)),
    ("odd_1", dict(rows=1081, cols=1920, nframes=1),
     dict(FEW, fused=0, dec_zero_kernel=1, dec_zero_list=0, dec="general", ccl="tw5")),
    ("odd_64", dict(rows=1081, cols=1921, nframes=64),
     dict(MANY, fused=0, dec="general", ccl="tw5", mask_scan=0, prescan=0)),
    ("thresh7_1024", dict(rows=1080, cols=1920, nframes=1024, adaptive_thresh=7),
     dict(MANY, fused=0, dec="wide", dec_xblocks=1, dec_yblocks=1, dec_band_rows=135, ccl="any", mask_scan=0, prescan=0)),
    ("unaligned_1024", dict(rows=1080, cols=1920, nframes=1024, row_stride=1922),
     dict(MANY, fused=0, bgr_direct=0, dec="unaligned", dec_xblocks=2, dec_yblocks=1, dec_band_rows=135, ccl="tw5", mask_scan=0, prescan=0)),
    ("unaligned_frames_1", dict(rows=1080, cols=1920, nframes=1, frames=0x10004),
     dict(FEW, fused=0, dec_zero_list=1, dec="unaligned", dec_xblocks=2, dec_yblocks=32, dec_band_rows=5)),
    ("bgr_1", dict(rows=1080, cols=1920, nframes=1, channels=3),
     dict(FEW, bgr_direct=0)),
    ("bgr_4_tail", dict(rows=1080, cols=1920, nframes=4, channels=3),  # the last chunk of a direct call: BGR frames take the fused sweep whatever their count
     dict(FEW, bgr_direct=0, **FUSED_1080, dec_zero_kernel=1, dec_zero_list=0)),
    ("bgr_1024", dict(rows=1080, cols=1920, nframes=1024, channels=3),
     dict(MANY, bgr_direct=1, **FUSED_1080, mask_scan=1, prescan=1)),
    ("bgr_1024_option_off", dict(rows=1080, cols=1920, nframes=1024, channels=3, bgr_direct=0),
     dict(bgr_direct=0, fused=1)),
    ("bgr_1024_unaligned", dict(rows=1080, cols=1920, nframes=1024, channels=3, row_stride=5768 + 4),
     dict(bgr_direct=0, fused=0, dec="unaligned")),
    ("bgr_1_fuse2", dict(rows=1080, cols=1920, nframes=1, channels=3, fuse_mode=2),
     dict(FEW, bgr_direct=1, fused=1)),
    ("fuse0_1024", dict(rows=1080, cols=1920, nframes=1024, fuse_mode=0),
     dict(MANY, fused=0, dec="wide", dec_xblocks=1, dec_yblocks=1, dec_band_rows=135, ccl="tw5", mask_scan=0, prescan=0)),
    ("fuse2_1", dict(rows=1080, cols=1920, nframes=1, fuse_mode=2),
     dict(FEW, **FUSED_1080, dec_zero_kernel=1, dec_zero_list=0)),
    ("fuse2_64", dict(rows=1080, cols=1920, nframes=64, fuse_mode=2),
     dict(MANY, **FUSED_1080, mask_scan=1, prescan=1)),
    ("wave_points_1", dict(rows=1080, cols=1920, nframes=1, wave_points=100),
     dict(FEW, big_points=100, all_wave=0, fork=1)),
    ("wave_points_1024", dict(rows=1080, cols=1920, nframes=1024, wave_points=100),
     dict(MANY, big_points=100)),
    ("expand_exact", dict(rows=1080, cols=1920, nframes=1024, expand_exact=1),
     dict(refprm=0)),
    ("no_subpix_1024", dict(rows=1080, cols=1920, nframes=1024, corner_subpix=0),
     dict(refine="none")),
    ("no_subpix_1", dict(rows=1080, cols=1920, nframes=1, corner_subpix=0),
     dict(refine="none", latency=1)),
]


@pytest.mark.parametrize("args,want", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_plan_table(args, want):
    plan = tk.chunk_plan(**args)
    got = {k: plan[k] for k in list(want) + list(CONSTANT)}
    assert got == dict(want, **CONSTANT)


def test_plan_reports_every_field():
    plan = tk.chunk_plan(1080, 1920, 1)
    assert tuple(plan) == tk.PLAN_FIELDS
