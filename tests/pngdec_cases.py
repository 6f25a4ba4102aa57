"""PNG files for the decoder tests (test_png_decode_host.py, test_png_decode_gpu.py, tools/pngdec_check.cpp's corpus), written by a
small writer of their own: struct, zlib.crc32, zlib.compressobj(level, DEFLATED, 15, 9, strategy), a filter type chosen per row; a
bit packer for the streams zlib never emits.  Every list is built once and cached; nobody modifies the arrays."""
import functools
import io
import struct
import zlib

import numpy as np

OK, EINVAL, EUNSUPPORTED = 0, -1, -5
SIG = b"\x89PNG\r\n\x1a\n"


def chunk(tag, data=b"", crc=None):
    c = zlib.crc32(tag + data) & 0xFFFFFFFF if crc is None else crc
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", c)


def ihdr(W, H, depth=8, ctype=0, interlace=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, ctype, 0, 0, interlace))


def filter_rows(a, filters):
    """uint8 (H,W) or (H,W,3) -> the filtered byte stream, row y with filter type filters[y]."""
    a = np.asarray(a, np.uint8)
    H = a.shape[0]
    bpp = 1 if a.ndim == 2 else a.shape[2]
    raw = a.reshape(H, -1).astype(np.int32)
    out = bytearray()
    zero = np.zeros_like(raw[0])
    for y in range(H):
        cur, up = raw[y], (raw[y - 1] if y else zero)
        left = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]]) if cur.size > bpp else np.zeros_like(cur)
        ul = np.concatenate([np.zeros(bpp, np.int32), up[:-bpp]]) if cur.size > bpp else np.zeros_like(cur)
        left, ul = left[:cur.size], ul[:cur.size]
        ft = int(filters[y])
        if ft == 0:
            pred = 0
        elif ft == 1:
            pred = left
        elif ft == 2:
            pred = up
        elif ft == 3:
            pred = (left + up) >> 1
        else:
            p = left + up - ul
            pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - ul)
            pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
        out.append(ft)
        out += ((cur - pred) & 255).astype(np.uint8).tobytes()
    return bytes(out)


ZLIB_SETTINGS = (("l0", 0, zlib.Z_DEFAULT_STRATEGY), ("l1", 1, zlib.Z_DEFAULT_STRATEGY), ("l6", 6, zlib.Z_DEFAULT_STRATEGY),
                 ("l9", 9, zlib.Z_DEFAULT_STRATEGY), ("huff", 6, zlib.Z_HUFFMAN_ONLY), ("rle", 6, zlib.Z_RLE), ("fixed", 6, zlib.Z_FIXED))


def deflate(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    return c.compress(raw) + c.flush()


def assemble(W, H, ctype, stream, split=None, before=(), after=(), empty_at=None, interlace=0, depth=8):
    """The file: IHDR, `before` chunks, the zlib stream cut into IDAT chunks of `split` bytes (None: one), `after` chunks, IEND."""
    parts = [stream] if not split else [stream[k:k + split] for k in range(0, len(stream), split)]
    if empty_at is not None:
        parts.insert(min(empty_at, len(parts)), b"")
    return SIG + ihdr(W, H, depth, ctype, interlace) + b"".join(before) + b"".join(chunk(b"IDAT", p) for p in parts) + b"".join(after) + chunk(b"IEND")


def make_png(a, filters=0, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, **kw):
    a = np.asarray(a, np.uint8)
    H, W = a.shape[:2]
    if np.isscalar(filters):
        filters = [filters] * H
    return assemble(W, H, 0 if a.ndim == 2 else 2, deflate(filter_rows(a, filters), level, strategy), **kw)


def synth(H, W, rgb, seed):
    """A structured page: flat paper, noise 0..5, dark boxes -- it compresses to dynamic blocks, not to stored ones."""
    r = np.random.RandomState(seed)
    a = np.full((H, W, 3 if rgb else 1), 200, np.int32)
    a += r.randint(0, 6, a.shape)
    for _ in range(max(1, H * W // 600)):
        y, x = r.randint(0, H), r.randint(0, W)
        h, w = r.randint(1, 12), r.randint(1, 30)
        a[y:y + h, x:x + w] = r.randint(10, 60, (1, 1, a.shape[2]))
    a = a.astype(np.uint8)
    return a if rgb else a[..., 0]


def pil_gray(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("L"))


SHAPES = ((1, 1), (1, 37), (33, 1), (70, 50), (64, 64), (65, 130), (129, 63), (203, 311), (300, 330))
FILTER_MODES = (0, 1, 2, 3, 4, "cycle", "random")


def _filters(mode, H, seed):
    if mode == "cycle":
        return [y % 5 for y in range(H)]
    if mode == "random":
        return list(np.random.RandomState(seed).randint(0, 5, H))
    return [mode] * H


@functools.lru_cache(None)
def matrix():
    """63 (name, file, expected L) covering every shape, both colour types, the seven filter modes and the seven zlib settings; the
    300 x 330 page meets all seven settings."""
    out = []
    for k in range(63):
        (H, W), rgb, mode = SHAPES[k % 9], bool(k % 2), FILTER_MODES[k % 7]
        zname, level, strategy = ZLIB_SETTINGS[(k + k // 9) % 7]
        a = synth(H, W, rgb, 100 + k)
        data = make_png(a, _filters(mode, H, k), level, strategy)
        out.append(("%dx%d-%s-f%s-%s" % (H, W, "rgb" if rgb else "gray", mode, zname), data, pil_gray(data)))
    return out


def block_types(stream):
    """The type of a zlib stream's first deflate block."""
    return (stream[2] >> 1) & 3


@functools.lru_cache(None)
def splits():
    from PIL import Image
    a, c = synth(70, 50, False, 7), synth(65, 130, True, 8)
    phys = chunk(b"pHYs", struct.pack(">IIB", 11811, 11811, 1))
    text = chunk(b"tEXt", b"Comment\0a scan")
    out = [("split1", make_png(a, _filters("cycle", 70, 0), split=1)),
           ("split7", make_png(c, _filters("random", 65, 1), split=7)),
           ("split7-empty-first", make_png(a, 4, split=7, empty_at=0)),
           ("split7-empty-mid", make_png(a, 3, split=7, empty_at=5)),
           ("split7-empty-last", make_png(a, 1, split=7, empty_at=10 ** 6)),
           ("ancillary", make_png(c, 2, split=7, before=(phys, text), after=(text,)))]
    for name, arr, kw in (("pil", a, {}), ("pil-opt", a, {"optimize": True}), ("pil-dpi", c, {"dpi": (300, 300)}), ("pil-rgb-opt", c, {"optimize": True})):
        buf = io.BytesIO()
        Image.fromarray(arr).save(buf, "PNG", **kw)
        out.append((name, buf.getvalue()))
    return [(n, d, pil_gray(d)) for n, d in out]


class Bits:
    """Deflate's bit order: Huffman codes most significant bit first, everything else least significant first."""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, n):
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, v, n):
        self.put(int(format(v, "0%db" % n)[::-1], 2), n)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def lit(self, s):                              # a literal/length symbol in the fixed code
        if s < 144:
            self.code(0x30 + s, 8)
        elif s < 256:
            self.code(0x190 + s - 144, 9)
        elif s < 280:
            self.code(s - 256, 7)
        else:
            self.code(0xC0 + s - 280, 8)

    def match(self, length, dist):
        LB = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
        LE = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
        DB = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
        DE = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
        k = max(i for i in range(29) if LB[i] <= length) if length < 258 else 28
        self.lit(257 + k)
        self.put(length - LB[k], LE[k])
        d = max(i for i in range(30) if DB[i] <= dist)
        self.code(d, 5)
        self.put(dist - DB[d], DE[d])


def fixed_stream(ops, final_stored=False, adler_of=None):
    """A zlib stream of one fixed-Huffman block from ops: an int is a literal, a (length, distance) pair a match."""
    b = Bits()
    b.put(0 if final_stored else 1, 1)
    b.put(1, 2)
    for op in ops:
        if isinstance(op, tuple):
            b.match(*op)
        else:
            b.lit(op)
    b.lit(256)
    if final_stored:
        b.put(1, 1)
        b.put(0, 2)
        b.align()
        b.put(0, 16)
        b.put(0xFFFF, 16)
    b.align()
    body = bytes(b.out)
    data = zlib.decompressobj(-15).decompress(body) if adler_of is None else adler_of
    return b"\x78\x01" + body + struct.pack(">I", zlib.adler32(data) & 0xFFFFFFFF)


@functools.lru_cache(None)
def hand_streams():
    """(name, file, expected): fixed-Huffman streams zlib never emits.  Each is first checked with zlib.decompress."""
    out = []
    r = np.random.RandomState(3)
    # a match (258, 32768): 130 rows of 1 + 255 bytes; the first 128 rows are literals, then the match, then literals
    rows = r.randint(0, 256, (128, 256))
    rows[:, 0] = 0
    head = [int(v) for v in rows.reshape(-1)]
    rest = [int(v) for v in r.randint(0, 256, 130 * 256 - 32768 - 258)]
    out.append(("far", 255, 130, fixed_stream(head + [(258, 32768)] + rest)))
    # (258, 1) and (3, 1): one row of 300 pixels
    out.append(("run", 300, 1, fixed_stream([0, 77, (258, 1), (3, 1)] + [int(v) for v in r.randint(0, 256, 300 - 1 - 261)])))
    # (4, 3): distance < length
    out.append(("overlap", 9, 1, fixed_stream([0, 1, 2, 3, (4, 3), 9, 8])))
    # a final empty stored block behind the data
    out.append(("empty-stored", 5, 2, fixed_stream([0, 1, 2, 3, 4, 5, 0, 5, 4, (3, 7)], final_stored=True)))
    res = []
    for name, W, H, stream in out:
        raw = zlib.decompress(stream)
        assert len(raw) == H * (W + 1), name
        a = np.frombuffer(raw, np.uint8).reshape(H, W + 1)
        assert not a[:, 0].any(), name
        res.append((name, assemble(W, H, 0, stream), a[:, 1:].copy()))
    return res


def adam7_raw(a):
    out = bytearray()
    for ys, xs, dy, dx in ((0, 0, 8, 8), (0, 4, 8, 8), (4, 0, 8, 4), (0, 2, 4, 4), (2, 0, 4, 2), (0, 1, 2, 2), (1, 0, 2, 1)):
        sub = a[ys::dy, xs::dx]
        if sub.size:
            for row in sub:
                out.append(0)
                out += row.tobytes()
    return bytes(out)


@functools.lru_cache(None)
def refusals():
    """(name, file): sound PNG files the decoder does not take."""
    from PIL import Image
    a = synth(20, 30, False, 11)
    c = synth(20, 30, True, 12)

    def save(img):
        buf = io.BytesIO()
        img.save(buf, "PNG")
        return buf.getvalue()
    out = [("gray16", save(Image.fromarray((a.astype(np.uint16) * 257)))),
           ("palette", save(Image.fromarray(c).convert("P"))),
           ("la", save(Image.fromarray(a).convert("LA"))),
           ("rgba", save(Image.fromarray(c).convert("RGBA"))),
           ("adam7", assemble(30, 20, 0, deflate(adam7_raw(a)), interlace=1)),
           ("bit1", save(Image.fromarray(a > 128))),
           ("trns", assemble(30, 20, 0, deflate(filter_rows(a, [0] * 20)), before=(chunk(b"tRNS", b"\x00\x10"),)))]
    return out


def dynamic_header_stream(cl_lens):
    """A zlib stream whose only block is a dynamic one with these 19 code-length code lengths (in the order of RFC 1951 3.2.7) and
    nothing usable behind them."""
    b = Bits()
    b.put(1, 1)
    b.put(2, 2)
    b.put(0, 5)
    b.put(0, 5)
    b.put(15, 4)
    for v in cl_lens:
        b.put(v, 3)
    b.put(0, 32)
    b.align()
    return b"\x78\x01" + bytes(b.out) + b"\0\0\0\1"


def container_ok(data):
    """The test's own container check: signature, IHDR first with length 13, critical CRCs, consecutive IDATs, IEND."""
    if data[:8] != SIG:
        return False
    pos, first, seen, closed = 8, True, False, False
    while True:
        if len(data) - pos < 12:
            return False
        n, tag = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        if n > len(data) - pos - 12:
            return False
        body = data[pos + 8:pos + 8 + n]
        if not (tag[0] & 32) and zlib.crc32(tag + body) & 0xFFFFFFFF != struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0]:
            return False
        if first != (tag == b"IHDR") or (tag == b"IHDR" and n != 13):
            return False
        if tag == b"IDAT":
            if closed:
                return False
            seen = True
        elif seen:
            closed = True
        if tag == b"IEND":
            return seen
        first = False
        pos += 12 + n


def idat_payload(data):
    pos, out = 8, b""
    while len(data) - pos >= 12:
        n, tag = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        if tag == b"IDAT":
            out += data[pos + 8:pos + 8 + n]
        pos += 12 + n
    return out


def is_corrupt(data, W, H, bpp):
    """What makes a member of the corrupt corpus corrupt, established without the decoder under test."""
    if not container_ok(data):
        return True
    try:
        raw = zlib.decompress(idat_payload(data))
    except zlib.error:
        return True
    stride = 1 + W * bpp
    if len(raw) != H * stride:
        return True
    return any(raw[y * stride] > 4 for y in range(H))


@functools.lru_cache(None)
def corrupt():
    """(name, file, W, H, bpp): every member must be refused with EINVAL."""
    a = synth(70, 50, False, 21)
    H, W = a.shape
    filt = _filters("cycle", H, 0)
    raw = filter_rows(a, filt)
    good = make_png(a, filt)
    stream = deflate(raw)
    out = []
    for k, n in enumerate((4, 20, 8 + 25 + 8 + len(stream) // 2, len(good) - 16, len(good) - 12)):
        out.append(("trunc%d" % k, good[:n]))
    flipped = bytearray(stream)
    flipped[len(stream) // 2] ^= 0x10
    out.append(("bitflip", assemble(W, H, 0, bytes(flipped))))
    out.append(("adler", assemble(W, H, 0, stream[:-4] + struct.pack(">I", (struct.unpack(">I", stream[-4:])[0] + 1) & 0xFFFFFFFF))))
    out.append(("oversubscribed", assemble(W, H, 0, dynamic_header_stream([1, 1, 1] + [0] * 16))))
    out.append(("incomplete", assemble(W, H, 0, dynamic_header_stream([1] + [0] * 18))))
    out.append(("too-far", assemble(W, H, 0, fixed_stream([0, (3, 2)] + [0] * (H * (W + 1) - 4), adler_of=bytes(H * (W + 1))))))
    out.append(("row-long", assemble(W, H, 0, deflate(raw + raw[-(W + 1):]))))
    out.append(("row-short", assemble(W, H, 0, deflate(raw[:-(W + 1)]))))
    five = bytearray(raw)
    five[(W + 1) * 33] = 5
    out.append(("filter5", assemble(W, H, 0, deflate(bytes(five)))))
    bad_crc = SIG + ihdr(W, H) + chunk(b"IDAT", stream, crc=(zlib.crc32(b"IDAT" + stream) ^ 1) & 0xFFFFFFFF) + chunk(b"IEND")
    out.append(("idat-crc", bad_crc))
    out.append(("no-iend", good[:-12]))
    return [(n, d, W, H, 1) for n, d in out]
