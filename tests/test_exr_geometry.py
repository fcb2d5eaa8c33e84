"""The EXR pack launch's geometry, without a GPU: rrt_exr_launch_geometry says which kernel a size takes and how the grid covers it,
and every size of the device tests (tests/exr_ref.py: GPU_CASES) still reaches the branch it is there for."""
import pytest

import exr_ref as xr


def _rrt():
    import relativisticraytracer_amd as rrt
    return rrt


def _geometry(fmt, case):
    rrt = _rrt()
    w, h, shift = case
    return rrt.exr_launch_geometry(rrt.ExrFormat(*fmt), w, h, shift)


@pytest.mark.parametrize("fmt", xr.FORMATS, ids="-".join)
def test_every_device_case_reaches_its_branch(fmt):
    for case in xr.WIDE_CASES + [xr.WRAP_CASE]:
        g = _geometry(fmt, case)
        assert g["wide"] and g["pixels"] == 8 and case[0] % 8 == 0, case
        assert g["grid"][0] * g["block"][0] * 8 >= case[0] > (g["grid"][0] - 1) * g["block"][0] * 8, case
    for case in xr.NARROW_CASES:
        g = _geometry(fmt, case)
        assert not g["wide"] and g["pixels"] == 1 and case[0] % 8 != 0, case
        assert g["grid"][0] * g["block"][0] >= 3 * case[0] > (g["grid"][0] - 1) * g["block"][0], case      # a thread per sample of a row
    w, h, shift = xr.OFFSET_CASE
    assert _geometry(fmt, (w, h, 0))["wide"] and not _geometry(fmt, xr.OFFSET_CASE)["wide"] and shift % 16 != 0
    for odd in (1, 4, 8, 15):          # any of the low four address bits
        assert not _geometry(fmt, (w, h, odd))["wide"]
    assert _geometry(fmt, (w, h, 32))["wide"]
    for case in xr.GPU_CASES:
        g = _geometry(fmt, case)
        assert g["threads"] == g["block"][0] * g["block"][1] and g["threads"] % 64 == 0 and g["block"][0] % 64 == 0
        rows = g["grid"][1] * g["block"][1]
        assert g["passes"] == -(-case[1] // rows) and (g["passes"] == 1) == (rows >= case[1]), case


@pytest.mark.parametrize("fmt", xr.FORMATS, ids="-".join)
def test_the_cases_cover_the_launch_paths_edges(fmt):
    g = {case: _geometry(fmt, case) for case in xr.GPU_CASES}
    # the row dimension wraps at WRAP_CASE -- and only just: sixteen rows into the second pass, none at the height one pass holds
    wrap = g[xr.WRAP_CASE]
    per_pass = wrap["grid"][1] * wrap["block"][1]
    assert wrap["passes"] == 2 and xr.WRAP_CASE[1] - per_pass == 16
    assert _geometry(fmt, (xr.WRAP_CASE[0], per_pass, 0))["passes"] == 1
    assert all(v["passes"] == 1 for case, v in g.items() if case != xr.WRAP_CASE)
    assert max(v["grid"][0] for v in g.values()) > 1 and max(v["grid"][1] for case, v in g.items() if case != xr.WRAP_CASE) > 1      # more than one workgroup each way
    heights = {case[1] for case in xr.GPU_CASES}
    assert {1, 16, 17, 33} <= heights                 # one row; one whole zip chunk; a short last chunk; two chunks and one row
    assert any(case[1] % g[case]["block"][1] for case in xr.GPU_CASES)      # a workgroup with rows past the frame's edge
    assert any((case[0] // 8) % g[case]["block"][0] for case in xr.WIDE_CASES)      # ... and with threads past a row's end
