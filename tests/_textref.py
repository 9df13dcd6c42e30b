"""The independent side of the file-layer tests: both file forms of a problem restated in pure Python / numpy, without the
library.  The .bal text as src/baproblem.rs:709-733 writes it and :580-629 reads it (every float through CPython's repr /
float: David Gay's shortest digits and correctly rounded strtod), the .bbal words of :736-764 by struct.pack, a layout
helper that puts chosen tokens at chosen byte offsets, and a restatement of what the device parser takes without
declining (csrc/text_kernels.hpp, csrc/decimal.hpp)."""
import functools
import math
import re
import struct
from decimal import Decimal

import numpy as np

WS = b" \n\t\r"


def rust_display(x):
    """Rust's `{}` of an f64: shortest round-trip digits, never an exponent"""
    x = float(x)
    if x != x:
        return "NaN"
    if math.isinf(x):
        return "inf" if x > 0 else "-inf"
    s = format(Decimal(repr(x)), "f")
    if "." in s:
        s = s.rstrip("0").rstrip(".")
    if s in ("0", "-0"):
        return "-0" if math.copysign(1.0, x) < 0 else "0"
    return s


def _display_all(a):
    """rust_display of every element of a float array, as a list (each distinct bit pattern is formatted once)"""
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    bits, inverse = np.unique(a.view(np.uint64), return_inverse=True)
    texts = [rust_display(v) for v in bits.view(np.float64).tolist()]
    return [texts[k] for k in inverse.tolist()]


def bal_text(bal9, pts, row_ptr, pt_idx, uv):
    """the .bal image of write_text (src/baproblem.rs:709-733): header, `cam pt u v` lines, nine values per camera line,
    three per point line"""
    bal9 = np.asarray(bal9, dtype=np.float64).reshape(-1, 9)
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    n_cam, n_pts, n_obs = len(bal9), len(pts), len(uv)
    assert len(row_ptr) == n_cam + 1 and int(row_ptr[-1]) == n_obs == len(pt_idx)
    cam_of = np.repeat(np.arange(n_cam), np.diff(np.asarray(row_ptr).astype(np.int64))).tolist()
    out = ["%d %d %d\n" % (n_cam, n_pts, n_obs)]
    t = _display_all(uv)
    out += ["%d %d %s %s\n" % (cam_of[o], int(pt_idx[o]), t[2 * o], t[2 * o + 1]) for o in range(n_obs)]
    t = _display_all(bal9)
    out += [" ".join(t[9 * c:9 * c + 9]) + "\n" for c in range(n_cam)]
    t = _display_all(pts)
    out += [" ".join(t[3 * p:3 * p + 3]) + "\n" for p in range(n_pts)]
    return "".join(out).encode("ascii")


def parse_bal_text(data):
    """(bal9, pts, row_ptr, pt_idx, uv) of a .bal image: the positional grammar of src/baproblem.rs:580-629 -- tokens split
    on space, newline, tab and carriage return; three counts, four tokens per observation, nine per camera, three per point;
    observations pushed onto their camera's list in file order (a stable sort by camera); what follows the last point is
    not read"""
    tok = data.split()                                        # bytes.split(): runs of ASCII whitespace
    assert b"\x0b" not in data and b"\x0c" not in data     # the two bytes split() takes for whitespace and the grammar does not
    n_cam, n_pts, n_obs = int(tok[0]), int(tok[1]), int(tok[2])
    k_cam = 3 + 4 * n_obs
    k_pts = k_cam + 9 * n_cam
    assert len(tok) >= k_pts + 3 * n_pts, "short file"
    cam = np.array([int(t) for t in tok[3:k_cam:4]], dtype=np.int64)
    pt = np.array([int(t) for t in tok[4:k_cam:4]], dtype=np.uint64)
    uv = np.array([float(t) for k in range(n_obs) for t in tok[5 + 4 * k:7 + 4 * k]], dtype=np.float64).reshape(-1, 2)
    if n_obs and (cam.max() >= n_cam or int(pt.max()) >= n_pts):
        raise IndexError("an observation's camera or point index is out of range")
    order = np.argsort(cam, kind="stable")
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(cam, minlength=n_cam))]).astype(np.uint64)
    bal9 = np.array([float(t) for t in tok[k_cam:k_pts]], dtype=np.float64).reshape(-1, 9)
    pts = np.array([float(t) for t in tok[k_pts:k_pts + 3 * n_pts]], dtype=np.float64).reshape(-1, 3)
    return bal9, pts, row_ptr, pt[order], uv[order]


def bbal_image(bal9, pts, row_ptr, pt_idx, uv):
    """the .bbal image of write_binary (src/baproblem.rs:736-764): big-endian words"""
    bal9 = np.asarray(bal9, dtype=np.float64).reshape(-1, 9)
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    out = [struct.pack(">QQQ", len(bal9), len(pts), len(uv))]
    for c in range(len(bal9)):
        a, b = int(row_ptr[c]), int(row_ptr[c + 1])
        out.append(struct.pack(">Q", b - a))
        out += [struct.pack(">Qdd", int(pt_idx[o]), uv[o, 0], uv[o, 1]) for o in range(a, b)]
    out += [struct.pack(">9d", *row) for row in bal9.tolist()] + [struct.pack(">3d", *row) for row in pts.tolist()]
    return b"".join(out)


def same_bits(a, b):
    """two problems' arrays (bal9, pts, row_ptr, pt_idx, uv) equal bit for bit"""
    for k, (x, y) in enumerate(zip(a, b)):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        if k in (2, 3):
            if not np.array_equal(x.astype(np.uint64), y.astype(np.uint64)):
                return False
        elif x.size != y.size or not np.array_equal(x.ravel().view(np.uint64), y.ravel().view(np.uint64)):
            return False
    return True


# ---- layout: tokens at chosen byte offsets -------------------------------------------------------------------------------
def bal_tokens(n_cam, n_pts, obs, cams, pts):
    """(tokens, separators) of a .bal file in the writer's own layout -- one space between the tokens of a line, one
    newline after it -- from token TEXTS: obs = [(cam, pt, u, v)], cams = nine texts per camera, pts = three per point"""
    tokens, seps = [str(n_cam), str(n_pts), str(len(obs))], [" ", " ", "\n"]
    for line, width in [(o, 4) for o in obs] + [(c, 9) for c in cams] + [(p, 3) for p in pts]:
        assert len(line) == width
        tokens += [str(t) for t in line]
        seps += [" "] * (width - 1) + ["\n"]
    return tokens, seps


def layout(tokens, seps=None, at=None, pad=" ", end=None):
    """The file of these tokens, token i followed by seps[i] (default: one space; the last one by `end`, default seps[-1]).
    at = {i: X}: token i starts at absolute byte offset X, which is met by inserting X - (where it would start) bytes of
    `pad`, repeated, in front of it.  Every constraint is asserted on the result."""
    seps = [" "] * len(tokens) if seps is None else list(seps)
    if end is not None:
        seps[-1] = end
    at = at or {}
    out, pos = [], 0
    for i, (t, s) in enumerate(zip(tokens, seps)):
        if i in at:
            assert pos <= at[i], "token %d cannot start at %d: the file is already %d bytes long" % (i, at[i], pos)
            out.append((pad * ((at[i] - pos) // len(pad) + 1))[:at[i] - pos])
            pos = at[i]
        out.append(t + s)
        pos += len(t) + len(s)
    data = "".join(out).encode("ascii")
    for i, x in at.items():
        t = tokens[i].encode("ascii")
        assert data[x:x + len(t)] == t and (x == 0 or data[x - 1] in WS), "token %d is not at %d" % (i, x)
        assert x + len(t) == len(data) or data[x + len(t)] in WS
    return data


def token_starts(data):
    """byte offsets at which a token starts (a non-whitespace byte at offset 0 or behind a whitespace byte)"""
    b = np.frombuffer(data, dtype=np.uint8)
    ws = (b == 32) | (b == 10) | (b == 9) | (b == 13)
    prev = np.concatenate([[True], ws[:-1]])
    return np.flatnonzero(~ws & prev)


def writer_tiles(data, n_cam, n_pts, n_obs, units=256):
    """Of an image in the writer's own layout: {"obs" | "cam" | "pts": [(offset, total) of every tile of `units` units]},
    a unit being an observation line, or one value of a camera / point line with the byte behind it"""
    b = np.frombuffer(data, dtype=np.uint8)
    nl = np.flatnonzero(b == 10)
    assert len(nl) == 1 + n_obs + n_cam + n_pts and (len(data) == 0 or data[-1:] == b"\n")
    ends = nl + 1                                             # the byte after every line
    sep = np.flatnonzero((b == 10) | (b == 32)) + 1
    blocks = {"obs": (ends[0], ends[1:1 + n_obs]), "cam": (ends[n_obs], sep[(sep > ends[n_obs]) & (sep <= ends[n_obs + n_cam])]),
              "pts": (ends[n_obs + n_cam], sep[sep > ends[n_obs + n_cam]])}
    assert len(blocks["cam"][1]) == 9 * n_cam and len(blocks["pts"][1]) == 3 * n_pts
    out = {}
    for name, (start, unit_end) in blocks.items():
        edge = np.concatenate([[start], unit_end]).astype(np.int64)
        first = edge[:-1][::units]
        last = np.concatenate([first[1:], edge[-1:]]) if len(first) else first
        out[name] = list(zip(first.tolist(), (last - first).tolist()))
    return out


# ---- what the device parser takes ---------------------------------------------------------------------------------------
_FLOAT = re.compile(r"[+-]?([0-9]+)(?:\.([0-9]+))?(?:[eE][+-]?[0-9]+)?\Z")
MAX_TOKEN, MAX_DIGITS = 400, 19                              # kParseLong; the digits a 64-bit significand holds


@functools.lru_cache(maxsize=None)
def accepts_float(t):
    """[+-]digits[.digits][(e|E)[+-]digits], at most MAX_TOKEN bytes, at most MAX_DIGITS significant digits.  Zeros in
    front of the first non-zero digit and behind the last one do not count: the parser keeps the first 19 digits from
    the first non-zero one on and declines only if a later digit is not zero."""
    m = _FLOAT.match(t)
    if m is None or len(t) > MAX_TOKEN:
        return False
    return len((m.group(1) + (m.group(2) or "")).lstrip("0").rstrip("0")) <= MAX_DIGITS


@functools.lru_cache(maxsize=None)
def accepts_index(t):
    """digits only, at most 19 of them"""
    return re.match(r"[0-9]{1,19}\Z", t) is not None


def rejected(data):
    """[(token number, text)] of the tokens of a .bal image that the device parser declines by this restatement (the
    header and what follows the last point are not the device's to parse).  must_accept(data) == not rejected(data)."""
    tok = [t.decode("ascii") for t in data.split()]
    n_cam, n_pts, n_obs = int(tok[0]), int(tok[1]), int(tok[2])
    k_cam = 3 + 4 * n_obs
    k_end = k_cam + 9 * n_cam + 3 * n_pts
    bad = []
    for k in range(3, min(k_end, len(tok))):
        is_index = k < k_cam and (k - 3) % 4 < 2
        if not (accepts_index(tok[k]) if is_index else accepts_float(tok[k])):
            bad.append((k, tok[k]))
    return bad


def must_accept(data):
    return not rejected(data)
