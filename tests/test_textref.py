"""The checker and the inputs of tests/test_gpu_text_edges.py, checked without a GPU: tests/_textref.py against the host
twins of the device file layer (city2ba_amd.baproblem.write_bal / read_bal / format_f64 / parse_f64), on every file the GPU
module generates, and the structural claim in each file's name -- "this tile's total is 24576 - s", "this token starts at
4096 t - k", "this tile holds 2048 token starts", "the only inversion is between observations 255 and 256" -- asserted on
the constructed bytes.  These assertions are what make the GPU cases mean what their names say."""
import numpy as np
import pytest

import _textref as T
import test_gpu_text_edges as G
from city2ba_amd.baproblem import format_f64, parse_f64, read_bal, write_bal


# ---- the checker itself --------------------------------------------------------------------------------------------------
def test_powers_of_ten_give_every_unit_length():
    """rust_display(10^k) is k + 1 characters for k = 0..308 and the host formatter agrees: values of 1..309 characters"""
    v = [float("1e%d" % k) for k in range(309)]
    assert [len(T.rust_display(x)) for x in v] == list(range(1, 310))
    assert format_f64(v) == [T.rust_display(x) for x in v]
    assert 256 * len(T.rust_display(1e94) + " ") == G.EMIT_CAP


def test_what_the_device_parser_accepts_restated():
    yes = ["0", "-0", "+1.5", "1e5", "1E-5", "12.5e+300", "0" * 391 + "12345.678", "1234567890123456789", "1" + "0" * 94,
           "0.0000000000000000000001234567890123456789", "1.50000000000000000000000000", "-1.2345678901234e-05"]
    no = ["NaN", "inf", "-inf", "1e", "--1", "1.5.2", "0x1p3", "12345678901234567891", "0.12345678901234567890123", "1_0"]
    narrower = [".5", "5."]                                    # the parser takes these; the restatement does not need them
    assert all(T.accepts_float(t) for t in yes) and not any(T.accepts_float(t) for t in no + narrower + ["", "0" * 392 + "12345.678"])
    vals, st = parse_f64(yes)
    assert (st == 0).all() and np.array_equal(vals.view(np.uint64), np.array([float(t) for t in yes]).view(np.uint64))
    assert (parse_f64(no)[1] != 0).all() and (parse_f64(narrower)[1] == 0).all()
    assert parse_f64(["0" * 391 + "12345.678"])[1][0] == 0 and len("0" * 391 + "12345.678") == G.PARSE_LONG
    assert all(T.accepts_index(t) for t in ["0", "007", "9" * 19]) and not any(T.accepts_index(t) for t in ["", "-1", "1.0", "9" * 20, "1e3"])


def test_layout_meets_or_refuses_its_constraints():
    data = T.layout(["1", "22", "333"], ["\n", " ", "\n"], at={1: 7, 2: 4096 - 1}, pad="\t \r\n")
    assert data[:2] == b"1\n" and data[7:9] == b"22" and data[4095:4098] == b"333" and len(data) == 4099
    assert set(data[2:7]) <= set(T.WS) and list(T.token_starts(data)) == [0, 7, 4095]
    with pytest.raises(AssertionError):
        T.layout(["1", "22"], at={1: 1})
    assert T.layout(["1", "2"], end="") == b"1 2"


def test_parse_bal_text_is_the_positional_grammar():
    data = b"2 1\t1\r\n1 0 0.5 -1e1\n" + b" ".join(b"%d" % k for k in range(18)) + b"\n7 8 9 left unread"
    bal9, pts, row_ptr, pt_idx, uv = T.parse_bal_text(data)
    assert bal9.tolist() == [list(map(float, range(9))), list(map(float, range(9, 18)))] and pts.tolist() == [[7.0, 8.0, 9.0]]
    assert row_ptr.tolist() == [0, 0, 1] and pt_idx.tolist() == [0] and uv.tolist() == [[0.5, -10.0]]
    with pytest.raises(IndexError):
        T.parse_bal_text(b"1 1 1\n1 0 0 0\n" + b"0 " * 12)


# ---- claims: what a file's name says, on its bytes -------------------------------------------------------------------------
def _tokens(data):
    starts = T.token_starts(data)
    tok = data.split()
    assert len(tok) == len(starts)
    return starts, tok


def _check(data, claims):
    starts, tok = _tokens(data)
    n_cam, n_pts, n_obs = int(tok[0]), int(tok[1]), int(tok[2])
    k_cam = 3 + 4 * n_obs
    k_end = k_cam + 9 * n_cam + 3 * n_pts
    tile = G.PARSE_TILE
    tiles = None
    for c in claims:
        kind = c[0]
        if kind in ("writer_tile", "last_tile", "window_cross", "tile_above_cap", "tile_below_cap", "tile_edge_texts"):
            tiles = tiles or T.writer_tiles(data, n_cam, n_pts, n_obs, G.TEXT_TILE)
            block = tiles[c[1]]
        if kind == "writer_tile":                               # this tile's offset is r mod 16 and its total is ...
            assert (block[c[2]][0] % 16, block[c[2]][1]) == (c[3], c[4]), c
        elif kind == "last_tile":
            assert len(block) == c[2] + 1, c
        elif kind == "window_cross":                            # offset residue x s, in full
            cross = {(off % 16, G.EMIT_CAP + c[2] - total) for off, total in block}
            assert cross >= {(r, s) for r in range(16) for s in range(16)}, c
        elif kind == "tile_above_cap":
            assert block[c[2]][1] > G.EMIT_CAP + 16, c
        elif kind == "tile_below_cap":
            assert block[c[2]][1] + 15 <= G.EMIT_CAP, c
        elif kind == "tile_edge_texts":
            units = tok[k_end - 3 * n_pts:k_end]
            assert (units[G.TEXT_TILE * c[2]].decode(), units[G.TEXT_TILE * c[2] + G.TEXT_TILE - 1].decode()) == (c[3], c[4]), c
        elif kind == "header":
            assert data.startswith(c[1].encode() + b"\n"), c
        elif kind == "index_widths":
            assert {len(t) for t in tok[3:k_cam:4]} == set(c[1]) and {len(t) for t in tok[4:k_cam:4]} == set(c[2]), c
        elif kind == "length":
            assert len(data) == c[1], c
        elif kind == "last_byte_is":
            assert (data[-1:] == b"\n") == (c[1] == "newline") and (data[-1] not in T.WS) == (c[1] == "token"), c
            assert len(tok) == k_end
        elif kind == "trailing_tiles_later":
            assert c[1] == k_end < len(tok) and starts[k_end] // tile - starts[k_end - 1] // tile == c[2], c
        elif kind == "token_at":                                # this token starts at ... and is m bytes long
            assert starts[c[1]] == c[2] and len(tok[c[1]]) == c[3], c
        elif kind == "last_token":
            assert len(tok[-1]) == c[1] and len(tok) == k_end and data[-1] not in T.WS, c
        elif kind == "tile_starts":                             # this tile holds ... token starts
            assert int(((starts >= tile * c[1]) & (starts < tile * (c[1] + 1))).sum()) == c[2], c
            assert len(data) >= tile * (c[1] + 1)
        elif kind == "phase":                                   # (k0 - 3) mod 4 of the deal of tokens to waves
            assert (int((starts < tile * c[1]).sum()) - 3) % 4 == c[2], c
        elif kind == "first_byte":
            b, is_start = data[tile * c[1]], tile * c[1] in starts
            assert {"token": is_start, "space": b in T.WS, "continues": b not in T.WS and not is_start}[c[2]], c
        elif kind == "bytes_at":
            assert data[c[1]:c[1] + len(c[2])] == c[2], c
        elif kind == "all_whitespace_bytes":
            assert all(bytes([w]) in data for w in T.WS)
        elif kind == "rank_in_tile":                            # token i is the rank-th token of tile t
            assert starts[c[1]] // tile == c[2] and c[1] - int((starts < tile * c[2]).sum()) == c[3], c
        elif kind == "index_out_of_range":
            last = k_cam - 4 + c[1]
            assert int(tok[last]) == (n_cam, n_pts)[c[1]]
            with pytest.raises(IndexError):
                T.parse_bal_text(data)
        elif kind == "passes":
            assert c[1] == n_cam and c[2] == {2: 1, 256: 1, 257: 2, 65536: 2, 65537: 3}[n_cam], c
        elif kind == "keys":
            cam = np.array([int(t) for t in tok[3:k_cam:4]])
            down = np.flatnonzero(cam[:-1] > cam[1:])
            name = c[1]
            if name.startswith("only-inversion-"):              # the only inversion is between observations a and a + 1
                a = int(name[len("only-inversion-"):].split("|")[0])
                assert down.tolist() == [a], c
            elif name == "reversed":
                assert (cam[:-1] >= cam[1:]).all()
            elif name == "all-equal-but-one":
                assert sorted(np.unique(cam, return_counts=True)[1].tolist())[0] == 1 and len(np.unique(cam)) == 2
            elif name == "64-low-bytes-per-chunk":
                assert all(len(set((cam[a:a + 64] & 255).tolist())) == len(cam[a:a + 64]) for a in range(0, len(cam), 64))
            elif name == "second-byte-only":
                assert not (cam & ~0xff00).any() and len(np.unique(cam)) > 1
            else:
                assert name == "random" and (len(down) > 0 or len(cam) <= 2)
        else:
            raise AssertionError("unknown claim %r" % (c,))


def _same(a, b):
    return T.same_bits(a, b)


@pytest.mark.parametrize("name", sorted(G.WRITER))
def test_writer_files_sit_where_their_names_say_and_the_host_writer_agrees(tmp_path, name):
    for f in G.WRITER[name]():
        want = T.bal_text(*f["arrays"])
        path = str(tmp_path / "host.bal")
        write_bal(path, *f["arrays"])
        assert open(path, "rb").read() == want, f["label"]
        assert f["claims"], f["label"]
        _check(want, f["claims"])


@pytest.mark.parametrize("name", sorted(G.READER))
def test_reader_files_sit_where_their_names_say_and_the_host_reader_agrees(tmp_path, name):
    for f in G.READER[name]():
        data = f["data"]
        assert f["claims"], f["label"]
        _check(data, f["claims"])
        bad = T.rejected(data)
        path = str(tmp_path / "in.bal")
        open(path, "wb").write(data)
        if f["host"] is not None:                              # well spelled, out of range: the host words the error
            assert not bad
            from city2ba_amd._lib import City2baError
            with pytest.raises(City2baError, match=f["host"]):
                read_bal(path)
            continue
        if f["decline"] is None:
            assert T.must_accept(data), (f["label"], bad[:3])
            tok = data.split()
            n_obs = int(tok[2])
            k_end = 3 + 4 * n_obs + 9 * int(tok[0]) + 3 * int(tok[1])
            floats = sorted({t.decode() for k, t in enumerate(tok[:k_end]) if k >= 3 + 4 * n_obs or (k >= 3 and (k - 3) % 4 >= 2)})
            for a in range(0, len(floats), 100_000):
                assert (parse_f64(floats[a:a + 100_000])[1] == 0).all(), f["label"]
        else:                                                  # exactly the intended token is declined
            assert [k for k, _ in bad] == [f["decline"]], (f["label"], bad[:3])
        assert _same(read_bal(path), T.parse_bal_text(data)), f["label"]


def test_every_case_the_issue_names_is_generated():
    assert {n for n in G.WRITER if n.startswith("window-")} == {"window-%s%+d" % (b, d) for b in ("pts", "obs") for d in (-1, 0, 1)}
    assert G.SHORT_TOTALS == (2, 3, 15, 16, 17, 31, 32, 33) and all("short-pts-%d" % n in G.WRITER for n in G.SHORT_TOTALS)
    assert {n for n in G.READER if n.startswith("straddle-")} == {"straddle-" + k for k in ("cam_idx", "pt_idx", "u", "v", "cam_value", "pt_value")}
    assert all("long-%d" % n in G.READER for n in (399, 400, 401))
    assert G.SORT_OBS == (2, 63, 64, 65, 2047, 2048, 2049, 4097) and G.SORT_CAMS == (2, 256, 257, 65536, 65537)
    assert [G.sort_passes(c) for c in G.SORT_CAMS] == [1, 1, 2, 2, 3]
    assert set(G.SORT_SHAPES) == {(n, 257) for n in G.SORT_OBS} | {(2049, c) for c in G.SORT_CAMS}
    assert all("sort-%d-%d" % s in G.READER for s in G.SORT_SHAPES)
    phases = set()
    for h in range(16, 24):
        (f,) = G.dense(h)
        phases.add((dict((c[0], c[-1]) for c in f["claims"])["phase"], dict((c[0], c[-1]) for c in f["claims"])["first_byte"]))
    assert phases == {(p, b) for p in range(4) for b in ("token", "space")}
    assert G.BBAL_CAMS == (0, 1, 255, 256, 257)


@pytest.mark.parametrize("with_obs", [True, False])
@pytest.mark.parametrize("n_cam", G.BBAL_CAMS)
def test_bbal_image_equals_the_host_writer(tmp_path, n_cam, with_obs):
    arrays = G.bbal_arrays(n_cam, with_obs)
    counts = np.diff(arrays[2].astype(np.int64))
    assert len(counts) == n_cam and (with_obs or len(arrays[4]) == 0) and (len(arrays[4]) > 0 or not with_obs or n_cam <= 2)
    if n_cam > 2:
        assert counts[0] == 0 and counts[-1] == 0                # an empty first and last camera
    path = str(tmp_path / "host.bbal")
    write_bal(path, *arrays)
    assert open(path, "rb").read() == T.bbal_image(*arrays)
    assert _same(read_bal(path), arrays)
