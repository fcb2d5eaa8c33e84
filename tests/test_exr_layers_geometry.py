"""The layers launch's geometry, without a GPU: rrt_exr_layers_launch_geometry says which kernel a layout takes, how the grid covers
it and how wide the filtered stores of its 4-byte channels are, and every size of the device tests (tests/exr_layers_ref.py) reaches
the branch it is named for -- the store-alignment case included: width % 16 == 8 with an odd number of HALF channels ahead of a FLOAT
channel."""
import numpy as np
import pytest

import exr_layers_ref as lr

FAKE = 0x7777000000000000          # made-up, 16-byte aligned addresses: nothing here reads them


def _rrt():
    import relativisticraytracer_amd as rrt
    return rrt


def _layers(rrt, set_name, w, h, compression, moved=None):
    """the set over made-up planes 2^32 bytes apart; moved: the plane whose address is 4 bytes off the 16-byte grid"""
    shapes = {"hdr": (4, 0, True), "rad": (4, 0, False), "pos": (3, 0, False), "vel": (3, 0, False), "steps": (1, 1, False), "hit": (1, 1, False)}
    planes = {k: ((FAKE + (i << 32) + (4 if k == moved else 0), words, kind), up) for i, (k, (words, kind, up)) in enumerate(shapes.items())}
    return lr.api_layers(rrt, lr.LAYER_SETS[set_name], planes, w, h, compression)


def _geometry(rrt, set_name, w, h, compression, payload=FAKE + (9 << 32), moved=None):
    L = _layers(rrt, set_name, w, h, compression, moved)
    return rrt.exr_layers_launch_geometry(L, L.address_bits(payload)), L


@pytest.mark.parametrize("compression", lr.COMPRESSIONS)
@pytest.mark.parametrize("set_name", sorted(lr.LAYER_SETS))
def test_every_device_case_reaches_its_branch(set_name, compression):
    rrt = _rrt()
    n_ch = len(lr.LAYER_SETS[set_name])
    for w, h in lr.WIDE_CASES + [lr.WRAP_CASE]:
        g, _ = _geometry(rrt, set_name, w, h, compression)
        assert g["wide"] in (1, 2) and g["pixels"] == 8 and w % 8 == 0, (w, h)
        assert g["grid"][0] * g["block"][0] * 8 >= w > (g["grid"][0] - 1) * g["block"][0] * 8, (w, h)
    for w, h in lr.NARROW_CASES:
        g, _ = _geometry(rrt, set_name, w, h, compression)
        assert g["wide"] is False and g["pixels"] == 1 and w % 8 != 0, (w, h)
        assert g["grid"][0] * g["block"][0] >= n_ch * w > (g["grid"][0] - 1) * g["block"][0], (w, h)      # a thread per sample of a row
    w, h = lr.MOVED_CASE
    assert _geometry(rrt, set_name, w, h, compression)[0]["wide"]
    assert _geometry(rrt, set_name, w, h, compression, payload=FAKE + (9 << 32) + 2)[0]["wide"] is False      # the payload 2 bytes off
    moved = lr.LAYER_SETS[set_name][-1][2]
    assert _geometry(rrt, set_name, w, h, compression, moved=moved)[0]["wide"] is False                       # one source 4 bytes off
    for w, h in lr.WIDE_CASES + lr.NARROW_CASES + [lr.MOVED_CASE, lr.WRAP_CASE]:
        g, _ = _geometry(rrt, set_name, w, h, compression)
        assert g["threads"] == g["block"][0] * g["block"][1] == 256 and g["block"][0] == 64
        rows = g["grid"][1] * g["block"][1]
        assert g["passes"] == -(-h // rows) and (g["passes"] == 1) == (rows >= h), (w, h)
    wrap, _ = _geometry(rrt, set_name, *lr.WRAP_CASE, compression)
    assert wrap["passes"] == 2 and lr.WRAP_CASE[1] - wrap["grid"][1] * wrap["block"][1] == 16      # sixteen rows into the second pass


def test_store_width_of_filtered_four_byte_channels():
    """out[6] = 2 exactly where a filtered layout mixes HALF and 4-byte channels and width % 16 == 8: there a 4-byte channel's place
    in a half of the chunk can be 8 past a multiple of 16 -- shown here from the layout itself, not from the library's flag"""
    rrt = _rrt()

    def misaligned(channels, w, rows):
        """does any 4-byte channel of any row of a `rows`-row filtered chunk start off the 16-byte grid, in either half?"""
        ordered = lr.ordered(channels)
        per_row = lr.bytes_per_pixel(ordered) // 2 * w
        for r in range(rows):
            at = r * per_row
            for _, t, _, _ in ordered:
                if t != "half" and (at % 16 or (at + rows * per_row) % 16):
                    return True
                at += (1 if t == "half" else 2) * w
        return False
    seen = set()
    for set_name, channels in lr.LAYER_SETS.items():
        mixed = len({t == "half" for _, t, _, _ in channels}) == 2
        for w in (8, 16, 24, 40, 64, 72):
            for compression in lr.COMPRESSIONS:
                g, _ = _geometry(rrt, set_name, w, 33, compression)
                want = 2 if (compression != "none" and mixed and w % 16 == 8) else 1
                assert g["wide"] == want, (set_name, w, compression)
                seen.add(want)
                if compression != "none" and g["wide"] == 1:         # 16-byte stores: every one of them must be aligned
                    assert not any(misaligned(channels, w, rows) for rows in (1, 16)), (set_name, w)
    assert seen == {1, 2}
    # the trap itself: one HALF channel ahead of a FLOAT channel at width 24 -- b.float starts 24 bytes into each half's row
    assert misaligned(lr.MIXED, 24, 1) and misaligned(lr.LAYER_SETS["all_half"], 72, 16)
    assert [t for _, t, _, _ in lr.ordered(lr.MIXED)][:2] == ["half", "float"]
    assert any(w % 16 == 8 for w, _ in lr.WIDE_CASES) and any(w % 16 == 0 for w, _ in lr.WIDE_CASES)
    # raw rows are always aligned: every channel's row starts on 16 bytes when width % 8 == 0
    for channels in lr.LAYER_SETS.values():
        at = 0
        for _, t, _, _ in lr.ordered(channels):
            assert (at * 8) % 16 == 0
            at += 2 if t == "half" else 4


def test_type_seams_of_the_mixed_set():
    """every type follows every other across a channel seam, the wrap from a row's last channel to the next row's first included"""
    types = [t for _, t, _, _ in lr.ordered(lr.MIXED)]
    pairs = set(zip(types, types[1:] + types[:1]))
    assert pairs == {(a, b) for a in ("half", "float", "uint") for b in ("half", "float", "uint") if a != b}
    assert np.array_equal(sorted(n for n, _, _, _ in lr.MIXED), [n for n, _, _, _ in lr.MIXED])
