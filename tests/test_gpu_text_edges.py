"""The sizes and offsets at which the device file layer can go wrong (csrc/text_kernels.hpp, the k_bbal_* kernels of
csrc/cell_kernels.hpp, csrc/capi_files.hpp), through public entries only (BAProblem.from_bal / write / from_file and the
options), against tests/_textref.py, byte for byte / bit for bit.  Every file is built to sit on a constant of those kernels;
tests/test_textref.py asserts on the bytes, without a GPU, that each file sits where its name says.

  writer   k_text_obs<EMIT> / k_text_vals<EMIT> / text_copy_out: a tile of 256 units goes through the LDS window iff
           total + shift <= kEmitCap (shift = the tile's address mod 16).  Tiles with total = kEmitCap - s, one more and one
           less, s = 0..15, each at all 16 residues of the tile's offset in the image (so total + shift meets the cap, cap + 1
           and cap - 1 whatever the image's own alignment is); a tile far above the cap between two that fit; last tiles of
           2, 3, 15, 16, 17, 31, 32, 33 bytes at all 16 residues (total < head, no whole 16-byte store, empty tail); blocks
           without units; NaN, inf, -inf, -0, 0 first and last in a tile; index widths; empty first and last camera.
  reader   k_text_count_tokens / k_text_parse: file lengths 16 j and 4096 t, one less and one more, with and without a final
           newline; tokens after the last point; a token of each of the six kinds straddling a tile edge at every split,
           and the whitespace byte on either side of the edge; tokens of 399 / 400 (accepted) and 401 bytes (declined)
           mid-tile, on a tile's last byte and last in the file; 2048 token starts in a tile at all four phases of the
           deal of tokens to waves; tiles without a token start; all four whitespace bytes, \\r\\n across an edge; the
           first camera / point value as token 256 q, 256 q - 1, 256 q + 1 of its tile; indices out of range.
  sort     k_text_check_sorted / k_sort_hist / k_sort_scatter / k_text_gather_obs: 2, 63, 64, 65, 2047, 2048, 2049, 4097
           observations, 2, 256, 257, 65536, 65537 cameras (1, 1, 2, 2, 3 passes); random, reversed, all keys equal but
           one, 64 distinct low bytes per chunk, keys that differ in the second byte only, and files whose ONLY inversion
           is between observations 0|1, 255|256 (two 256-thread blocks of the check) or n - 2|n - 1.
  .bbal    0, 1, 255, 256, 257 cameras, an empty first and last camera, no observations.

The cases follow kTextTile = 256, kEmitCap = 24576, kParseTile = 4096, kParseOver = 448, kParseLong = 400 and
kSortTile = 2048; if those constants change, these follow them.  Not covered: four sort passes (more than 2^24 cameras)
and files of 4 GiB or more."""
import numpy as np
import pytest

import _textref as T

pytestmark = pytest.mark.gpu

TEXT_TILE, EMIT_CAP = 256, 24 * 1024                         # kTextTile, kEmitCap
PARSE_TILE, PARSE_OVER, PARSE_LONG = 4096, 448, 400          # kParseTile, kParseOver, kParseLong
SORT_TILE, CHECK_BLOCK = 2048, 256                           # kSortTile, the block of k_text_check_sorted


# ======================================================================================================================
# generators: pure Python / numpy, no library.  A writer file is a dict(label, arrays, claims), a reader file a
# dict(label, data, claims, decline, host); claims are tuples that tests/test_textref.py checks on the bytes.
# ======================================================================================================================
def _value_of_length(n):
    """a double whose text has n characters (1 <= n <= 309): a power of ten"""
    assert 1 <= n <= 309
    return float("1e%d" % (n - 1))


_ONE_CAMERA = np.array([[0.0, 0.0, 0.0, 1.0, 2.0, 3.0, 1.0, 0.0, 0.0]])


def _arrays(bal9, pts, row_ptr, pt_idx, uv):
    return (np.asarray(bal9, dtype=np.float64).reshape(-1, 9), np.asarray(pts, dtype=np.float64).reshape(-1, 3),
            np.asarray(row_ptr, dtype=np.uint64), np.asarray(pt_idx, dtype=np.uint64), np.asarray(uv, dtype=np.float64).reshape(-1, 2))


def _points_of_units(unit_len):
    """a point block whose units (value + separator) have these lengths, padded with 2-byte units to whole points"""
    unit_len = list(unit_len) + [2] * (-len(unit_len) % 3)
    return np.array([_value_of_length(n - 1) for n in unit_len]).reshape(-1, 3)


def _point_block_start(n_units):
    """offset of the point block's first byte: one camera, no observations, n_units values (padded to whole points)"""
    return len("1 %d 0\n" % ((n_units + 2) // 3)) + len("0 0 0 1 2 3 1 0 0\n")


def _point_file(label, tiles, claims):
    """one camera, no observations, and a point block made of these tiles (lists of unit lengths)"""
    pts = _points_of_units([n for t in tiles for n in t])
    return dict(label=label, arrays=_arrays(_ONE_CAMERA, pts, [0, 0], [], np.zeros((0, 2))), claims=claims)


def _filler(units, pos, residue):
    """a tile of `units` 2-byte units, one of them longer, after which the offset is `residue` mod 16"""
    t = [2] * units
    t[units // 2] += (residue - (pos + 2 * units)) % 16
    return t


def window_points(d):
    """point tiles of total kEmitCap + d - s, s = 0..15, each at every residue r of its offset, a short tile in front of
    each setting the residue"""
    tiles, claims, pos = [], [], _point_block_start(2 * 256 * TEXT_TILE)
    for r in range(16):
        for s in range(16):
            f = _filler(TEXT_TILE, pos, r)
            tile = [96] * TEXT_TILE
            tile[(16 * r + s) % TEXT_TILE] += d - s
            claims += [("writer_tile", "pts", len(tiles) + 1, r, EMIT_CAP + d - s)]
            tiles += [f, tile]
            pos += sum(f) + sum(tile)
    return [_point_file("window-pts%+d" % d, tiles, claims + [("window_cross", "pts", d)])]


def _obs_lines(lines, n_pts, label, claims):
    """three cameras, the first and the last without observations; lines = [(point, length of u, length of v)]"""
    pt = [p for p, _, _ in lines]
    uv = [[_value_of_length(a), _value_of_length(b)] for _, a, b in lines]
    bal9 = np.repeat(_ONE_CAMERA, 3, axis=0)
    pts = (np.arange(3 * n_pts) % 7).astype(np.float64).reshape(-1, 3)
    return dict(label=label, arrays=_arrays(bal9, pts, [0, 0, len(lines), len(lines)], pt, uv), claims=claims)


def _obs_len(p, lu, lv):
    return 1 + 1 + len(str(p)) + 1 + lu + 1 + lv + 1           # "1 p u v\n"


def _obs_tile(total, n_lines, n_pts, salt):
    """n_lines observation lines of `total` bytes together: point indices of every width, u and v of about equal length"""
    pt = [(37 * (salt + j)) % n_pts for j in range(n_lines)]
    each = total // n_lines
    lines = [(p, (each - len(str(p)) - 5) // 2, (each - len(str(p)) - 5) - (each - len(str(p)) - 5) // 2) for p in pt]
    k = salt % n_lines
    p, lu, lv = lines[k]
    lines[k] = (p, lu + total - each * n_lines, lv)
    assert sum(_obs_len(*ln) for ln in lines) == total and all(ln[1] >= 1 and ln[2] >= 1 for ln in lines)
    return lines


def window_obs(d):
    """the same cross through k_text_obs"""
    n_pts, n_obs = 1000, 2 * 256 * TEXT_TILE
    lines, claims, pos = [], [], len("3 %d %d\n" % (n_pts, n_obs))
    for r in range(16):
        for s in range(16):
            pad = (r - (pos + 8 * TEXT_TILE)) % 16
            f = [(0, 1, 1)] * (TEXT_TILE - 1) + [(0, 1 + pad, 1)]
            tile = _obs_tile(EMIT_CAP + d - s, TEXT_TILE, n_pts, 16 * r + s)
            claims += [("writer_tile", "obs", len(lines) // TEXT_TILE + 1, r, EMIT_CAP + d - s)]
            lines += f + tile
            pos += sum(_obs_len(*ln) for ln in f) + EMIT_CAP + d - s
    assert len(lines) == n_obs
    return [_obs_lines(lines, n_pts, "window-obs%+d" % d, claims + [("window_cross", "obs", d)])]


SHORT_TOTALS = (2, 3, 15, 16, 17, 31, 32, 33)


def short_points(total):
    """the last tile of the point block is `total` bytes long, at every residue of its offset"""
    last = [total] if total < 4 else [2, total - 2]
    full = next(m for m in (1, 2, 3) if (TEXT_TILE * m + len(last)) % 3 == 0)
    files = []
    for r in range(16):
        tiles = [[5] * TEXT_TILE for _ in range(full - 1)]
        tiles += [_filler(TEXT_TILE, _point_block_start(TEXT_TILE * full + len(last)) + sum(map(sum, tiles)), r), last]
        files.append(_point_file("short-pts-%d@%d" % (total, r), tiles, [("writer_tile", "pts", full, r, total), ("last_tile", "pts", full)]))
    return files


def short_obs(total):
    """the same for the observation block (a line is 8 bytes at least, so the totals start at 15)"""
    n_pts = 12
    last = [total] if total < 16 else [8, total - 8]
    files = []
    for r in range(16):
        pos = len("3 %d %d\n" % (n_pts, TEXT_TILE + len(last)))
        pad = (r - (pos + 8 * TEXT_TILE)) % 16
        lines = [(0, 1, 1)] * (TEXT_TILE - 1) + [(0, 1 + pad, 1)]
        lines += [(11 if n > 8 else 3, n - 6 - len(str(11 if n > 8 else 3)), 1) for n in last]
        files.append(_obs_lines(lines, n_pts, "short-obs-%d@%d" % (total, r),
                                [("writer_tile", "obs", 1, r, total), ("last_tile", "obs", 1)]))
    return files


def empty_blocks():
    none = np.zeros((0, 2))
    pts = np.arange(12.0).reshape(4, 3)
    bal9 = np.repeat(_ONE_CAMERA, 2, axis=0)
    return [dict(label="no-observations", arrays=_arrays(bal9, pts, [0, 0, 0], [], none), claims=[("header", "2 4 0")]),
            dict(label="no-cameras", arrays=_arrays(np.zeros((0, 9)), pts, [0], [], none), claims=[("header", "0 4 0")]),
            dict(label="no-points", arrays=_arrays(bal9, np.zeros((0, 3)), [0, 0, 0], [], none), claims=[("header", "2 0 0")]),
            dict(label="nothing", arrays=_arrays(np.zeros((0, 9)), np.zeros((0, 3)), [0], [], none), claims=[("header", "0 0 0")])]


SPECIALS = (float("nan"), float("inf"), float("-inf"), -0.0, 0.0)


def special_widths():
    """NaN, inf, -inf, -0 and 0 as the first and as the last unit of a tile, in the point block and as u / v of the first
    and last line of an observation tile; wild bit patterns between them"""
    rng = np.random.default_rng(501)
    n = len(SPECIALS)
    vals = rng.integers(0, 2**64, TEXT_TILE * n + 1, dtype=np.uint64).view(np.float64).copy()
    uv = rng.integers(0, 2**64, 2 * TEXT_TILE * n, dtype=np.uint64).view(np.float64).copy().reshape(-1, 2)
    for k, x in enumerate(SPECIALS):
        vals[TEXT_TILE * k] = x
        vals[TEXT_TILE * k + TEXT_TILE - 1] = SPECIALS[(k + 1) % n]
        uv[TEXT_TILE * k] = (x, SPECIALS[(k + 2) % n])
        uv[TEXT_TILE * k + TEXT_TILE - 1] = (SPECIALS[(k + 3) % n], x)
    n_obs = len(uv)
    claims = [("tile_edge_texts", "pts", k, T.rust_display(x), T.rust_display(SPECIALS[(k + 1) % n])) for k, x in enumerate(SPECIALS)]
    return [dict(label="specials", arrays=_arrays(np.repeat(_ONE_CAMERA, 3, axis=0), vals.reshape(-1, 3), [0, 0, n_obs, n_obs],
                                                  np.arange(n_obs) % (len(vals) // 3), uv), claims=claims)]


def neighbours():
    """a tile far above the cap (256 values of 301 characters; 256 lines of 610 bytes) between two that fit: the direct
    and the LDS path in neighbouring workgroups"""
    tiles = [[90] * TEXT_TILE, [302] * TEXT_TILE, [90] * TEXT_TILE]
    lines = [(5, 40, 40)] * TEXT_TILE + [(7, 301, 301)] * TEXT_TILE + [(9, 40, 40)] * (TEXT_TILE - 3)
    f = _obs_lines(lines, 10, "neighbours", [])
    bal9, _, row_ptr, pt_idx, uv = f["arrays"]
    claims = [("tile_above_cap", "pts", 1), ("tile_below_cap", "pts", 0), ("tile_below_cap", "pts", 2),
              ("tile_above_cap", "obs", 1), ("tile_below_cap", "obs", 0), ("tile_below_cap", "obs", 2)]
    return [dict(label="neighbours", arrays=_arrays(bal9, _points_of_units([n for t in tiles for n in t]), row_ptr, pt_idx, uv), claims=claims)]


def obs_indices():
    """camera and point indices of every width the counts allow (1-2 and 1-6 digits), u and v chosen for length, the
    first and the last camera empty"""
    n_cam, n_pts = 12, 100_001
    pt = [0, 9, 10, 99, 100, 999, 1000, 9999, 10_000, 99_999, 100_000]
    per = 60
    cam_of = np.repeat(np.arange(1, n_cam - 1), per)
    pt_idx = np.array([pt[(o * 7 + o // per) % len(pt)] for o in range(len(cam_of))])
    uv = np.array([[_value_of_length(1 + (o * 13) % 309), -_value_of_length(1 + (o * 29) % 309)] for o in range(len(cam_of))])
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(cam_of, minlength=n_cam))])
    pts = (np.arange(3 * n_pts) % 10).astype(np.float64).reshape(-1, 3)
    return [dict(label="obs-indices", arrays=_arrays(np.repeat(_ONE_CAMERA, n_cam, axis=0), pts, row_ptr, pt_idx, uv),
                 claims=[("index_widths", (1, 2), (1, 2, 3, 4, 5, 6))])]


WRITER = {}
for _d in (-1, 0, 1):
    WRITER["window-pts%+d" % _d] = (lambda d=_d: window_points(d))
    WRITER["window-obs%+d" % _d] = (lambda d=_d: window_obs(d))
for _n in SHORT_TOTALS:
    WRITER["short-pts-%d" % _n] = (lambda n=_n: short_points(n))
    if _n >= 15:
        WRITER["short-obs-%d" % _n] = (lambda n=_n: short_obs(n))
WRITER.update({"empty-blocks": empty_blocks, "specials": special_widths, "neighbours": neighbours, "obs-indices": obs_indices})


# ---- reader ------------------------------------------------------------------------------------------------------------
_SPELL = ("%r", "%.17g", "%+.13e", "%.6f", "%.3g")


def _base(n_cam, n_pts, n_obs, seed, spell=_SPELL, sorted_cams=True):
    """token texts of a small problem: (n_cam, n_pts, obs, cams, pts) for _textref.bal_tokens"""
    rng = np.random.default_rng(seed)
    cam = rng.integers(0, n_cam, n_obs)
    if sorted_cams:
        cam = np.sort(cam)

    def text(k):
        v = float(rng.normal() * 10.0 ** int(rng.integers(-3, 4)))
        return spell[k % len(spell)] % v
    obs = [(int(c), int(rng.integers(0, n_pts)), text(2 * o), text(2 * o + 1)) for o, c in enumerate(cam)]
    cams = [[text(9 * c + j) for j in range(9)] for c in range(n_cam)]
    pts = [[text(3 * p + j + 1) for j in range(3)] for p in range(n_pts)]
    return n_cam, n_pts, obs, cams, pts


def _reader_file(label, data, claims, decline=None, host=None):
    """decline = None: the device parses the file.  decline = the number of the one token it must decline; host = None: the
    host parser then reads the file, host = a pattern: the host parser's error"""
    return dict(label=label, data=data, claims=claims, decline=decline, host=host)


def lengths(unit):
    """file lengths unit * j - 1, unit * j, unit * j + 1 with a final newline and with the last token on the last byte;
    tokens after the last point in the same tile and three tiles later"""
    b = _base(5, 9, (12 if unit == 16 else 150), seed=600 + unit)
    tokens, seps = T.bal_tokens(*b)
    natural = len(T.layout(tokens, seps))
    target = unit * (natural // unit + 1)
    files = []
    for n in (target - 1, target, target + 1):
        for end in ("\n", ""):
            last = len(tokens) - 1
            data = T.layout(tokens, seps, at={last: n - len(tokens[last]) - len(end)}, end=end)
            files.append(_reader_file("length-%d%s" % (n, "-newline" if end else "-token-last"), data,
                                      [("length", n), ("last_byte_is", "newline" if end else "token")]))
    for far in (0, 3):
        more = ["trailing", "tokens", "1e", "--", "2"]
        k = len(tokens)
        at = {k: PARSE_TILE * (len(T.layout(tokens, seps)) // PARSE_TILE + far) + 77} if far else None
        data = T.layout(tokens + more, seps + [" "] * len(more), at=at, pad=" \n\t\r", end="")
        files.append(_reader_file("trailing-%d-tiles-later" % far, data, [("trailing_tiles_later", k, far)]))
    return files


STRADDLE = {"cam_idx": 19, "pt_idx": 19, "u": 20, "v": 20, "cam_value": 20, "pt_value": 20}


def straddle(kind):
    """every token of this kind is m bytes long; one of them starts at 4096 t - k for k = 0..m, t = k + 1: k = 1..m - 1 are the
    splits of the token across the edge, k = 0 and k = m put the whitespace byte before / behind it on the edge"""
    m = STRADDLE[kind]
    sizes = {"cam_value": (640, 9, 10), "pt_value": (6, 2100, 10)}.get(kind, (60, 90, 2600))
    n_cam, n_pts, obs, cams, pts = _base(*sizes, seed=700 + m + len(kind))
    rng = np.random.default_rng(701)

    def fixed():
        t = "%+.13e" % float(rng.normal() * 10.0 ** int(rng.integers(-9, 10)))
        assert len(t) == 20
        return t
    if kind == "cam_idx":
        obs = [("%019d" % c, p, u, v) for c, p, u, v in obs]
    elif kind == "pt_idx":
        obs = [(c, "%019d" % p, u, v) for c, p, u, v in obs]
    elif kind == "u":
        obs = [(c, p, fixed(), v) for c, p, u, v in obs]
    elif kind == "v":
        obs = [(c, p, u, fixed()) for c, p, u, v in obs]
    elif kind == "cam_value":
        cams = [[fixed() for _ in row] for row in cams]
    else:
        pts = [[fixed() for _ in row] for row in pts]
    tokens, seps = T.bal_tokens(n_cam, n_pts, obs, cams, pts)
    k_cam = 3 + 4 * len(obs)
    k_pts = k_cam + 9 * n_cam
    cand = {"cam_idx": range(3, k_cam, 4), "pt_idx": range(4, k_cam, 4), "u": range(5, k_cam, 4), "v": range(6, k_cam, 4),
            "cam_value": range(k_cam, k_pts), "pt_value": range(k_pts, len(tokens))}[kind]
    cand = np.array(cand)
    nat = np.concatenate([[0], np.cumsum([len(t) + len(s) for t, s in zip(tokens, seps)])])[:-1]
    at, shift, claims = {}, 0, []
    for k in range(m + 1):
        x = PARSE_TILE * (k + 1) - k
        i = int(cand[nat[cand] + shift <= x][-1])
        assert len(tokens[i]) == m and i not in at and x - (nat[i] + shift) < 256
        at[i] = x
        shift = x - nat[i]
        claims.append(("token_at", i, x, m))
    return [_reader_file("straddle-" + kind, T.layout(tokens, seps, at=at), claims)]


def _long_token(n):
    return "0" * (n - 9) + "12345.678"


def long_tokens(n):
    """a token of n bytes (19 significant digits or fewer: leading zeros) mid-tile, on a tile's last byte (the bytes up to
    4096 + n - 1 of the overhang are then needed), and last in the file"""
    assert n + 1 <= PARSE_OVER                                # the token and the byte behind it lie in the staged overhang
    files = []
    for where in ("mid-tile", "tile-last-byte", "file-last"):
        n_cam, n_pts, obs, cams, pts = _base(4, 11, 260, seed=800 + n)
        tokens, seps = T.bal_tokens(n_cam, n_pts, obs, cams, pts)
        nat = np.concatenate([[0], np.cumsum([len(t) + len(s) for t, s in zip(tokens, seps)])])[:-1]
        if where == "file-last":
            i, at, claims = len(tokens) - 1, None, [("last_token", n)]
        else:
            x = 2 * PARSE_TILE - 1 if where == "tile-last-byte" else PARSE_TILE + 1500
            i = max(k for k in range(5, 3 + 4 * len(obs), 4) if nat[k] <= x)                  # a u
            at, claims = {i: x}, [("token_at", i, x, n)]
        tokens[i] = _long_token(n)
        data = T.layout(tokens, seps, at=at, end="" if where == "file-last" else None)
        files.append(_reader_file("long-%d-%s" % (n, where), data, claims, decline=i if n > PARSE_LONG else None))
    return files


def dense(h):
    """`c p u v` lines of one-digit tokens from byte h on: 2048 token starts in tile 1.  h = 16..23 gives every phase
    (k0 - 3) mod 4 of the deal with the tile's first byte starting a token (h even) and being whitespace (h odd)"""
    n_cam, n_pts, n_obs = 10, 10, 1700
    rng = np.random.default_rng(900 + h)
    cam = rng.integers(0, n_cam, n_obs) if h % 4 < 2 else np.sort(rng.integers(0, n_cam, n_obs))
    obs = [(int(c), int(rng.integers(0, 10)), int(rng.integers(0, 10)), int(rng.integers(0, 10))) for c in cam]
    cams = [[int(rng.integers(0, 10)) for _ in range(9)] for _ in range(n_cam)]
    pts = [[int(rng.integers(0, 10)) for _ in range(3)] for _ in range(n_pts)]
    tokens, seps = T.bal_tokens(n_cam, n_pts, obs, cams, pts)
    data = T.layout(tokens, seps, at={3: h})
    return [_reader_file("dense-%d" % h, data, [("tile_starts", 1, PARSE_TILE // 2), ("tile_starts", 2, PARSE_TILE // 2),
                                                ("phase", 1, (PARSE_TILE - h + 1) // 2 % 4), ("first_byte", 1, "token" if h % 2 == 0 else "space")])]


def dense_continued():
    """the same with a two-digit token on bytes 4095 | 4096: the tile's first byte continues a token"""
    files = []
    for h in (17, 19, 21, 23):
        f = dense(h)[0]
        tok = f["data"].split()
        n_obs = int(tok[2])
        k = int(np.searchsorted(T.token_starts(f["data"]), PARSE_TILE - 1))
        assert T.token_starts(f["data"])[k] == PARSE_TILE - 1 and 3 <= k < 3 + 4 * n_obs
        data = f["data"][:PARSE_TILE - 1] + b"0" + f["data"][PARSE_TILE - 1:]
        files.append(_reader_file("dense-continued-%d" % h, data, [("token_at", k, PARSE_TILE - 1, 2), ("first_byte", 1, "continues"),
                                                                   ("tile_starts", 1, PARSE_TILE // 2 - 1)]))
    return files


def whitespace_runs():
    """runs of all four whitespace bytes that leave one tile, then two consecutive tiles, without a token start, in the
    observation block and in the point block; \\r\\n across a tile edge"""
    n_cam, n_pts, obs, cams, pts = _base(6, 40, 120, seed=950)
    tokens, seps = T.bal_tokens(n_cam, n_pts, obs, cams, pts)
    k_pts = 3 + 4 * len(obs) + 9 * n_cam
    nat = np.concatenate([[0], np.cumsum([len(t) + len(s) for t, s in zip(tokens, seps)])])[:-1]
    a = max(k for k in range(3, 3 + 4 * len(obs)) if nat[k] < PARSE_TILE - 100)
    at = {a + 1: 2 * PARSE_TILE + 3}                         # tile 1 is empty
    b = a + 60
    at[b] = 3 * PARSE_TILE - 1 - len(tokens[b])              # token b, then \r on 3 * 4096 - 1 and \n on 3 * 4096
    seps[b] = "\r\n"
    c = k_pts + 31
    at[c] = 6 * PARSE_TILE                                    # tiles 4 and 5 are empty; a token starts on the tile's first byte
    data = T.layout(tokens, seps, at=at, pad="\t \r\n")
    return [_reader_file("whitespace-runs", data, [("tile_starts", 1, 0), ("tile_starts", 4, 0), ("tile_starts", 5, 0),
                                                   ("bytes_at", 3 * PARSE_TILE - 1, b"\r\n"), ("all_whitespace_bytes",)])]


def block_boundary(block):
    """the first camera / point value is token 256 q - 1, 256 q, 256 q + 1 of its tile (q = 1, 2): the deal of tokens to
    lanes changes kind inside a group of 256, on its edge, and one past it"""
    files = []
    for rank in (255, 256, 257, 511, 512, 513):
        n_cam, n_pts, n_obs = (40, 30, 140) if block == "cam" else (45, 30, 40)
        b = _base(n_cam, n_pts, n_obs, seed=1000 + rank, spell=("%.3g", "%.1f"))
        tokens, seps = T.bal_tokens(*b)
        first = 3 + 4 * n_obs + (0 if block == "cam" else 9 * n_cam)
        data = T.layout(tokens, seps, at={first - rank: PARSE_TILE}, pad=" \n")
        files.append(_reader_file("first-%s-value-is-token-%d" % (block, rank), data, [("rank_in_tile", first, 1, rank)]))
    return files


def out_of_range():
    files = []
    for field, words in ((0, "cam_i < cams.len"), (1, "p_i < points.len")):
        n_cam, n_pts, obs, cams, pts = _base(7, 13, 300, seed=1100 + field)
        last = list(obs[-1])
        last[field] = (n_cam, n_pts)[field]
        obs[-1] = tuple(last)
        tokens, seps = T.bal_tokens(n_cam, n_pts, obs, cams, pts)
        files.append(_reader_file("index-out-of-range-%d" % field, T.layout(tokens, seps), [("index_out_of_range", field)],
                                  decline=3 + 4 * (len(obs) - 1) + field, host=words))
    return files


# ---- sort ----------------------------------------------------------------------------------------------------------------
SORT_OBS = (2, 63, 64, 65, SORT_TILE - 1, SORT_TILE, SORT_TILE + 1, 2 * SORT_TILE + 1)
SORT_CAMS = (2, 256, 257, 65536, 65537)
SORT_SHAPES = [(n, 257) for n in SORT_OBS] + [(SORT_TILE + 1, c) for c in SORT_CAMS if c != 257]


def sort_passes(n_cam):
    bits = 1
    while bits < 32 and (n_cam - 1) >> bits:
        bits += 1
    return (bits + 7) // 8


def _single_inversion(n_obs, n_cam, i):
    a = (np.arange(n_obs) * n_cam) // n_obs
    if a[i] == a[i + 1]:
        if a[i] + 1 <= n_cam - 1:
            a[i + 1:] = np.maximum(a[i + 1:], a[i] + 1)
        else:
            a[:i + 1] = np.minimum(a[:i + 1], a[i + 1] - 1)
    a[i], a[i + 1] = a[i + 1], a[i]
    return a


def sort_keys(n_obs, n_cam):
    """{pattern: camera index of every observation, in file order}"""
    rng = np.random.default_rng(1200 + n_obs + n_cam)
    rnd = rng.integers(0, n_cam, n_obs)
    keys = {"random": rnd, "reversed": np.sort(rnd)[::-1].copy()}
    one = np.full(n_obs, n_cam - 1)
    one[n_obs // 2] = 0
    keys["all-equal-but-one"] = one
    i = np.arange(n_obs)
    if n_cam >= 256:
        low = (3 * (i % 64) + i // 64) % 256
        keys["64-low-bytes-per-chunk"] = low + 256 * ((i // 7) % (n_cam // 256)) if n_cam > 256 else low
    if n_cam > 256:
        keys["second-byte-only"] = 256 * rng.integers(0, min(256, -(-n_cam // 256)), n_obs)
    for at in sorted({0, n_obs - 2} | ({CHECK_BLOCK - 1} if n_obs > CHECK_BLOCK else set())):
        keys["only-inversion-%d|%d" % (at, at + 1)] = _single_inversion(n_obs, n_cam, at)
    return keys


def sort_files(n_obs, n_cam):
    n_pts = 7
    tail = "0 0 0 0 0 0 1 0 0\n" * n_cam + "".join("%d 0.5 -%d\n" % (p, p) for p in range(n_pts))
    files = []
    for name, cam in sort_keys(n_obs, n_cam).items():
        assert cam.min() >= 0 and cam.max() < n_cam and len(cam) == n_obs
        body = "".join("%d %d %d.5 -%d.25\n" % (c, (5 * o) % n_pts, o, o) for o, c in enumerate(cam.tolist()))
        claims = [("passes", n_cam, sort_passes(n_cam)), ("keys", name)]
        files.append(_reader_file("sort-%d-%d-%s" % (n_obs, n_cam, name), ("%d %d %d\n" % (n_cam, n_pts, n_obs) + body + tail).encode("ascii"), claims))
    return files


READER = {"length-16": lambda: lengths(16), "length-4096": lambda: lengths(PARSE_TILE), "dense-continued": dense_continued,
          "whitespace-runs": whitespace_runs, "first-camera-value": lambda: block_boundary("cam"),
          "first-point-value": lambda: block_boundary("pts"), "out-of-range": out_of_range}
for _k in STRADDLE:
    READER["straddle-" + _k] = (lambda k=_k: straddle(k))
for _n in (PARSE_LONG - 1, PARSE_LONG, PARSE_LONG + 1):
    READER["long-%d" % _n] = (lambda n=_n: long_tokens(n))
for _h in range(16, 24):
    READER["dense-%d" % _h] = (lambda h=_h: dense(h))
for _o, _c in SORT_SHAPES:
    READER["sort-%d-%d" % (_o, _c)] = (lambda o=_o, c=_c: sort_files(o, c))


# ---- .bbal ---------------------------------------------------------------------------------------------------------------
BBAL_CAMS = (0, 1, 255, 256, 257)


def bbal_arrays(n_cam, with_obs):
    """n_cam cameras (the first and the last without observations), 23 points"""
    rng = np.random.default_rng(1300 + n_cam)
    n_pts = 23
    counts = rng.integers(0, 9, n_cam) if with_obs else np.zeros(n_cam, dtype=np.int64)
    if n_cam > 2:
        counts[0] = counts[-1] = 0
    n_obs = int(counts.sum())
    bal9 = np.column_stack([np.zeros((n_cam, 3)), rng.uniform(-50, 50, (n_cam, 3)), rng.uniform(0.8, 1.2, n_cam), rng.uniform(-1e-2, 1e-2, (n_cam, 2))])
    uv = rng.integers(0, 2**64, 2 * n_obs, dtype=np.uint64).view(np.float64).reshape(-1, 2)
    return _arrays(bal9, rng.normal(size=(n_pts, 3)), np.concatenate([[0], np.cumsum(counts)]), rng.integers(0, n_pts, n_obs), uv)


# ======================================================================================================================
# the device
# ======================================================================================================================
@pytest.fixture(scope="module")
def c2b():
    import __graft_entry__ as entry
    entry.build()
    import city2ba_amd
    assert city2ba_amd.device_count() > 0
    try:
        yield city2ba_amd
    finally:
        city2ba_amd.reset_default_options()


def _state(ba):
    return ba.cameras_bal(), ba.points(), ba.row_ptr, ba.pt_idx, ba.observations()


@pytest.mark.parametrize("name", sorted(WRITER))
def test_device_text_image_at_the_writer_edges(c2b, tmp_path, name):
    for k, f in enumerate(WRITER[name]()):
        arrays = f["arrays"]
        ba = c2b.BAProblem.from_bal(*arrays)
        assert ba.options()["host_text"] == 0
        assert T.same_bits(_state(ba), arrays), f["label"]    # the file holds the cameras as they were given
        path = tmp_path / ("w%d.bal" % k)
        ba.write(str(path))
        ba.close()
        got, want = path.read_bytes(), T.bal_text(*arrays)
        assert len(got) == len(want), f["label"]
        assert got == want, (f["label"], next(i for i, (x, y) in enumerate(zip(got, want)) if x != y))


@pytest.mark.parametrize("name", sorted(READER))
def test_device_text_reader_at_the_reader_edges(c2b, tmp_path, name):
    for k, f in enumerate(READER[name]()):
        path = tmp_path / ("r%d.bal" % k)
        path.write_bytes(f["data"])
        c2b.set_default_options(text_device_min_bytes=0, text_device_strict=True)     # the device's own result, or an error
        if f["decline"] is None:
            ba = c2b.BAProblem.from_file(str(path))
            assert T.same_bits(_state(ba), T.parse_bal_text(f["data"])), f["label"]
            ba.close()
            continue
        with pytest.raises(c2b.City2baError, match="declined"):
            c2b.BAProblem.from_file(str(path))
        c2b.set_default_options(text_device_strict=False)
        if f["host"] is None:                                  # the host parser reads what the device declined
            ba = c2b.BAProblem.from_file(str(path))
            assert T.same_bits(_state(ba), T.parse_bal_text(f["data"])), f["label"]
            ba.close()
        else:
            with pytest.raises(c2b.City2baError, match=f["host"]):
                c2b.BAProblem.from_file(str(path))


@pytest.mark.parametrize("with_obs", [True, False])
@pytest.mark.parametrize("n_cam", BBAL_CAMS)
def test_device_bbal_image_at_the_block_edges(c2b, tmp_path, n_cam, with_obs):
    arrays = bbal_arrays(n_cam, with_obs)
    ba = c2b.BAProblem.from_bal(*arrays)
    assert T.same_bits(_state(ba), arrays)
    path = tmp_path / "dev.bbal"
    ba.write(str(path))
    ba.close()
    assert path.read_bytes() == T.bbal_image(*arrays)
    back = c2b.BAProblem.from_file(str(path))
    assert T.same_bits(_state(back), arrays)
    back.close()
