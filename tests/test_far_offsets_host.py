"""The plan of the far-offset tests (tests/farcases.py), checked without a GPU:
every call holds more than 2^31 pixels, every threshold a buffer can reach is
straddled by a probe, the ragged marks are inside images, and the peak device
memory stays within the cap. tests/test_gpu_far_offsets.py runs the plan."""
import pytest

import farcases as fc

PLANS = fc.all_plans()
IDS = [f"{e}-{fc.variant_id(v)}-{c.name}" for e, v, c in PLANS]


def test_the_cases_are_the_documented_ones():
    assert (fc.ALIGNED.W, fc.ALIGNED.H, fc.ALIGNED.n) == (256, 128, 65539)
    assert (fc.RAGGED.W, fc.RAGGED.H, fc.RAGGED.n) == (253, 131, 64797)
    # aligned: the 2^30 and 2^31 pixel marks are image starts, every vector form applies
    assert (1 << 30) % fc.ALIGNED.image_pixels == 0 and (1 << 31) % fc.ALIGNED.image_pixels == 0
    assert fc.ALIGNED.W % 16 == 0 and not fc.marks_inside_images(fc.ALIGNED)
    # ragged: no vector form applies (odd W: rows of f32 vectors are not 16-byte aligned,
    # no row is a multiple of 4 bytes), the marks are inside images
    assert fc.RAGGED.W % 2 == 1 and fc.RAGGED.image_pixels % 2 == 1 and fc.marks_inside_images(fc.RAGGED)
    # the 4:2:0 entry points refuse odd sides: their ragged case is even, W no multiple of
    # 4 (so W / 2 is odd: no aligned chroma row) or of the 16-pixel strip
    assert fc.EVEN.W % 2 == 0 and fc.EVEN.H % 2 == 0 and fc.EVEN.W % 4 and fc.marks_inside_images(fc.EVEN)
    assert set(fc.cases_of("flow_warp_u8")) == {"aligned", "ragged"}
    assert set(fc.cases_of("frames_to_yuv420_u8")) == {"aligned", "even"}
    # more fields than the y extent of a launch (65,535)
    assert fc.COLOR.n > 65535 and (fc.COLOR.W, fc.COLOR.H) == (16, 8)


def test_every_entry_point_has_a_plan():
    assert set(fc.VARIANTS) == {
        "flow_color", "flow_convert", "flow_consistency", "flow_warp_u8", "flow_interp_u8", "flow_compose", "flow_advect_points",
        "flow_fill", "flow_fit_motion", "motion_to_flow", "warp_motion_u8", "flow_fit_homography",
        "homography_to_flow", "warp_homography_u8", "temporal_denoise_u8", "frames_to_gray_u8",
        "yuv420_to_frames_u8", "frames_to_yuv420_u8"}
    assert all(len(v) >= 1 for v in fc.VARIANTS.values())
    # padded source strides once in every family that takes them
    for e in ("flow_warp_u8", "flow_interp_u8", "warp_motion_u8", "warp_homography_u8", "temporal_denoise_u8",
              "frames_to_gray_u8", "yuv420_to_frames_u8", "frames_to_yuv420_u8"):
        assert sum(v[-1] is True for v in fc.VARIANTS[e]) == 1, e
    assert len(PLANS) == len(set(IDS))


@pytest.mark.parametrize("entry,variant,case", PLANS, ids=IDS)
def test_plan(entry, variant, case):
    bufs = fc.plan(entry, variant, case)
    assert case.pixels > 1 << 31 and case.pixels < 1 << 32
    assert fc.peak_bytes(case, bufs) + fc.TEMPORARIES <= fc.MEMORY_CAP
    probes = fc.probe_images(case, bufs)
    assert probes == sorted(set(probes)) and probes[0] == 0 and probes[-1] == case.n - 1
    assert {1, case.n - 2} <= set(probes) and len(probes) <= 64
    reached = 0
    for b in bufs:
        total = b.bytes(case.n)
        # every threshold the buffer reaches, in bytes, in its elements and (a per-pixel buffer) in pixels ...
        px = b.image_bytes // case.image_pixels if b.image_bytes % case.image_pixels == 0 else 1
        for size in {1, b.elem, px}:
            for t in fc.thresholds(total // size):
                first, last = (t * size - 1) // b.image_bytes, (t * size) // b.image_bytes
                # ... is straddled: the images holding the last unit below it and the first at it are probes,
                # and so are the images before and after the one that contains it
                assert {first, last} <= set(probes), (b.name, size, t)
                assert {max(last - 1, 0), min(last + 1, case.n - 1)} <= set(probes), (b.name, size, t)
                reached += 1
        # what crossings() lists is what the loop above found
        assert all(0 <= img < case.n for _, _, img in fc.crossings(case, b))
    # a per-pixel buffer of at least one byte a pixel crosses 2^31 bytes: no plan is without a threshold
    assert reached >= 1
    if case.name != "aligned":
        assert fc.marks_inside_images(case)
        for b in bufs:
            for _, t, img in fc.crossings(case, b):
                if b.image_bytes % case.image_pixels == 0:  # a per-pixel buffer: the mark is no image start
                    unit = {"byte": 1, "element": b.elem, "pixel": b.image_bytes // case.image_pixels}
                    assert any((t * s) % b.image_bytes for s in unit.values()), (b.name, t)


def test_thresholds_and_crossings():
    assert fc.thresholds(1 << 31) == [] and fc.thresholds((1 << 31) + 1) == [1 << 31]
    assert fc.thresholds((1 << 33) + 1) == [1 << 31, 1 << 32, 2 << 32]
    c = fc.ALIGNED
    b = fc.flow("f", c, fc.F32)  # 8 bytes a pixel, 4 an element: 2^34 bytes and a bit
    got = {(u, t) for u, t, _ in fc.crossings(c, b)}
    assert ("byte", 1 << 31) in got and ("byte", 3 << 32) in got and ("byte", 4 << 32) in got
    assert ("element", 1 << 31) in got and ("element", 1 << 32) in got and ("pixel", 1 << 31) in got
    # the 2^31 pixel mark of the aligned case is the start of image 65536
    assert [i for u, t, i in fc.crossings(c, b) if (u, t) == ("pixel", 1 << 31)] == [65536]
    assert fc.fill_cells(1, 1) == 0 and fc.fill_cells(2, 2) == 1 and fc.fill_cells(5, 3) == 3 * 2 + 2 * 1 + 1
