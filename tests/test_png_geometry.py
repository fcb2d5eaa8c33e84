"""Without a GPU: from rrt_png_launch_geometry and the header's constants, the frames tests/test_gpu_png.py launches still reach the
branches they are there for -- every stride residue, a band boundary, a row of several segments, more chunks than a workgroup has
threads, more than one workgroup on both paths -- and the launch's LDS stays within 64 KiB."""
import numpy as np

import png_ref as pr


def _sizes(rrt):
    wide, narrow = rrt.png_launch_geometry(None, 64, 64), rrt.png_launch_geometry(None, 64, 64, 1)
    assert wide["wide"] and not narrow["wide"]
    return pr.gpu_sizes(wide["rows"], wide["threads"], narrow["threads"]), wide, narrow


def test_the_constants_are_the_headers():
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd import png
    _, wide, narrow = _sizes(rrt)
    assert wide["rows"] == png.BAND_ROWS and wide["threads"] == 256 and narrow["threads"] == narrow["rows"] == 64
    for depth in (8, 16):
        g = rrt.png_launch_geometry(rrt.PngFormat(depth), 1 << 20, 2)
        assert g["segment_chunks"] == png.SEGMENT_CHUNKS and g["lds_bytes"] == 2 * (16 * png.SEGMENT_CHUNKS + 160) <= 65536 - 256


def test_gpu_sizes_reach_their_branches():
    import relativisticraytracer_amd as rrt
    sizes, wide, narrow = _sizes(rrt)
    for depth in (8, 16):
        f = rrt.PngFormat(depth)
        g = {name: rrt.png_launch_geometry(f, w, h) for name, (w, h) in sizes.items()}
        assert g["one pixel"]["grid"] == 1 and g["one pixel"]["chunks"] == 2
        residues = {rrt.png_frame_bytes(f, w, h, layout=True)[1] % 16 for name, (w, h) in sizes.items() if name.startswith("width")}
        assert residues == (set(range(16)) if depth == 8 else set(range(1, 16, 2)))
        assert all(h > 1 for name, (w, h) in sizes.items() if name.startswith("width"))      # rows start at every alignment, not row 0 alone
        w, h = sizes["two bands plus a row"]
        assert h == 2 * wide["rows"] + 1 and g["two bands plus a row"]["grid"] == 3
        assert g["a row of several segments"]["segments"] > 1 and g["a row of several segments"]["chunks"] > g["a row of several segments"]["segment_chunks"]
        assert all(v["segments"] == 1 for name, v in g.items() if name != "a row of several segments")
        many = g["more chunks than threads"]
        assert many["chunks"] > wide["threads"] and many["segments"] == 1 and many["grid"] == 2
        rows = sizes["more rows than a narrow workgroup"]
        assert rrt.png_launch_geometry(f, *rows, 1)["grid"] == 3 and g["more rows than a narrow workgroup"]["grid"] > 1
        assert all(v["lds_bytes"] <= 65536 - 256 and v["wide"] for v in g.values())
        for name in pr.NARROW_SIZES:
            for bits in (1, 4, 15):
                n = rrt.png_launch_geometry(f, *sizes[name], bits)
                assert not n["wide"] and n["lds_bytes"] == 0 and n["grid"] == -(-sizes[name][1] // narrow["rows"])


def test_chunks_cover_every_start_of_a_row():
    """the most chunks a row's span touches, from the definition: a row that starts 15 bytes past a 16-byte word"""
    import relativisticraytracer_amd as rrt
    for depth, bpp in ((8, 3), (16, 6)):
        for w in (1, 2, 5, 21, 36, 1400, 16384):
            stride = 1 + w * bpp
            most = max(-(-(a + stride) // 16) for a in range(16))
            assert rrt.png_launch_geometry(rrt.PngFormat(depth), w, 3)["chunks"] == most == int(np.ceil((15 + stride) / 16))
