"""CPU: the library's PNG decoder (ebo_decode_png8 / ebo_read_png8, csrc/png8.h) -- what cv::imread(path, CV_8U) returns
for a DAVIS frame, without OpenCV or zlib in the library.

* the three golden frames decode to what tests/frontend_ref.read_png_gray8 (Python's zlib) reads;
* random images round-trip bit for bit over the five row filters (per image and mixed per row), zlib levels 0-9, the
  strategies Z_FILTERED / Z_HUFFMAN_ONLY / Z_RLE / Z_FIXED (stored, fixed and dynamic blocks all occur), IDAT chunks
  of 1 byte, 100 bytes and one whole, and the sizes 1x1, 1xN, Nx1 and odd widths;
* every other bit depth and colour type, Adam7 and a preset dictionary are EBO_ERR_UNSUPPORTED naming the property;
* malformed input is EBO_ERR_ARG: each truncation of a small PNG, a seeded sample of byte flips, bad checksums, a
  stream short of (or past) h * (w + 1) bytes, a side beyond 16384; the same cases run through csrc/png8.h built
  under AddressSanitizer + UBSan (tests/cpp/png8_fuzz.cpp)."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import frontend_ref

HERE = os.path.dirname(os.path.abspath(__file__))
CPP = os.path.join(HERE, "cpp")

STRATEGIES = {"default": None, "filtered": zlib.Z_FILTERED, "huffman_only": zlib.Z_HUFFMAN_ONLY, "rle": zlib.Z_RLE,
              "fixed": zlib.Z_FIXED}


def _image(rng, h, w):
    """Half smooth ramps (long matches, runs), half noise (literals)."""
    y, x = np.mgrid[0:h, 0:w]
    smooth = (x * 3 + y * 5) % 256
    noise = rng.integers(0, 256, size=(h, w))
    mask = rng.random((h, w)) < 0.5
    return np.where(mask, smooth, noise).astype(np.uint8)


def _chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)


def _png(ihdr, stream, extra=b""):
    return b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", ihdr) + extra + _chunk(b"IDAT", stream) + _chunk(b"IEND", b"")


def _raw_rows(img):
    return b"".join(b"\x00" + row.tobytes() for row in img)


def _first_block_type(png):
    """BTYPE of the first deflate block of a single-IDAT PNG written by synth.png8_bytes."""
    pos, stream = 8, b""
    while pos < len(png):
        n, kind = struct.unpack(">I4s", png[pos:pos + 8])
        if kind == b"IDAT":
            stream += png[pos + 8:pos + 8 + n]
        pos += 12 + n
    return (stream[2] >> 1) & 3


def test_golden_frames_equal_the_python_reader(ebo):
    for path in frontend_ref.FRAMES:
        a = ebo.read_png8(path)
        assert a.dtype == np.uint8 and a.shape == (180, 240)
        assert np.array_equal(a, frontend_ref.read_png_gray8(path))
        assert np.array_equal(ebo.decode_png8(open(path, "rb").read()), a)


@pytest.mark.parametrize("shape", [(1, 1), (1, 57), (43, 1), (7, 5), (17, 33), (180, 240)])
@pytest.mark.parametrize("filters", [0, 1, 2, 3, 4, "mixed"])
def test_round_trip_sizes_and_filters(ebo, synth, shape, filters):
    rng = np.random.default_rng(hash((shape, str(filters))) & 0xFFFF)
    img = _image(rng, *shape)
    f = rng.integers(0, 5, size=shape[0]) if filters == "mixed" else filters
    for split in (1, 100, None):
        png = synth.png8_bytes(img, filters=f, idat_split=split)
        assert np.array_equal(ebo.decode_png8(png), img), (shape, filters, split)


@pytest.mark.parametrize("strategy", sorted(STRATEGIES))
def test_round_trip_levels_strategies_and_idat_splits(ebo, synth, strategy):
    rng = np.random.default_rng(7)
    img = _image(rng, 23, 37)
    rows = rng.integers(0, 5, size=23)
    for level in range(10):
        for filters in (0, 4, rows):
            for split in (1, 100, None):
                png = synth.png8_bytes(img, filters=filters, level=level, strategy=STRATEGIES[strategy], idat_split=split)
                assert np.array_equal(ebo.decode_png8(png), img), (level, split)


def test_all_three_block_types_occur(ebo, synth):
    """Stored (level 0), fixed (Z_FIXED) and dynamic (default, compressible data) blocks, each decoded."""
    img = _image(np.random.default_rng(3), 64, 64)
    seen = set()
    for level, strategy in ((0, None), (6, zlib.Z_FIXED), (6, None), (9, zlib.Z_HUFFMAN_ONLY)):
        png = synth.png8_bytes(img, filters=1, level=level, strategy=strategy)
        seen.add(_first_block_type(png))
        assert np.array_equal(ebo.decode_png8(png), img)
    assert seen == {0, 1, 2}


def test_size_query_and_capacity(ebo, synth, tmp_path):
    import ctypes as C
    png = synth.png8_bytes(_image(np.random.default_rng(1), 9, 13))
    w, h = C.c_int32(), C.c_int32()
    f = ebo.lib().ebo_decode_png8
    assert f(png, C.c_size_t(len(png)), C.byref(w), C.byref(h), None, C.c_size_t(0)) == ebo.OK
    assert (w.value, h.value) == (13, 9)
    small = np.zeros(13 * 9 - 1, dtype=np.uint8)
    assert f(png, C.c_size_t(len(png)), C.byref(w), C.byref(h), ebo._vp(small), C.c_size_t(small.size)) == ebo.ERR_RANGE
    path = tmp_path / "x.png"
    path.write_bytes(png)
    assert np.array_equal(ebo.read_png8(path), ebo.decode_png8(png))
    with pytest.raises(ebo.EboError) as e:
        ebo.read_png8(tmp_path / "missing.png")
    assert e.value.code == ebo.ERR_ARG and "missing.png" in str(e.value)


UNSUPPORTED = [
    ("depth1", (1, 0, 0), "bit depth 1"),
    ("depth2", (2, 0, 0), "bit depth 2"),
    ("depth4", (4, 0, 0), "bit depth 4"),
    ("depth16", (16, 0, 0), "bit depth 16"),
    ("rgb", (8, 2, 0), "colour type 2"),
    ("palette", (8, 3, 0), "colour type 3"),
    ("grey_alpha", (8, 4, 0), "colour type 4"),
    ("rgba", (8, 6, 0), "colour type 6"),
    ("adam7", (8, 0, 1), "Adam7"),
]


@pytest.mark.parametrize("name,fmt,words", UNSUPPORTED, ids=[u[0] for u in UNSUPPORTED])
def test_unsupported_formats_name_the_property(ebo, name, fmt, words):
    depth, ctype, interlace = fmt
    w, h = 4, 3
    ihdr = struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, interlace)
    png = _png(ihdr, zlib.compress(b"\x00" * (h * (w * 8 + 1))))
    with pytest.raises(ebo.EboError) as e:
        ebo.decode_png8(png)
    assert e.value.code == ebo.ERR_UNSUPPORTED, str(e.value)
    assert words in str(e.value)


def test_preset_dictionary_is_unsupported(ebo):
    w, h = 5, 4
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_DEFAULT_STRATEGY, zdict=b"\x00\x01\x02\x03" * 8)
    stream = co.compress(_raw_rows(np.zeros((h, w), np.uint8))) + co.flush()
    with pytest.raises(ebo.EboError) as e:
        ebo.decode_png8(_png(struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0), stream))
    assert e.value.code == ebo.ERR_UNSUPPORTED and "preset dictionary" in str(e.value)


def _malformed():
    img = _image(np.random.default_rng(5), 6, 7)
    h, w = img.shape
    ihdr = struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0)
    raw = _raw_rows(img)
    good = zlib.compress(raw)
    bad_adler = good[:-4] + struct.pack(">I", (zlib.adler32(raw) + 1) & 0xFFFFFFFF)
    png = _png(ihdr, good)
    bad_crc = bytearray(png)
    bad_crc[8 + 8 + 13] ^= 1  # IHDR's CRC
    filt = bytearray(raw)
    filt[0] = 5
    return {
        "adler": (_png(ihdr, bad_adler), "Adler-32"),
        "crc": (bytes(bad_crc), "CRC-32"),
        "short_stream": (_png(ihdr, zlib.compress(raw[:-1])), "short"),
        "long_stream": (_png(ihdr, zlib.compress(raw + b"\x00")), "more image data"),
        "filter_type": (_png(ihdr, zlib.compress(bytes(filt))), "filter"),
        "wide": (_png(struct.pack(">IIBBBBB", 16385, 1, 8, 0, 0, 0, 0), good), "16384"),
        "tall": (_png(struct.pack(">IIBBBBB", 1, 16385, 8, 0, 0, 0, 0), good), "16384"),
        "zero": (_png(struct.pack(">IIBBBBB", 0, 3, 8, 0, 0, 0, 0), good), "size"),
        "no_idat": (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", ihdr) + _chunk(b"IEND", b""), "IDAT"),
        "no_iend": (png[:-12], "truncated"),
        "unknown_critical": (_png(ihdr, good, extra=_chunk(b"ABCD", b"xyz")), "unknown critical chunk"),
        "signature": (b"\x89PNG\r\n\x1a\x0b" + png[8:], "signature"),
        "block_type_3": (_png(ihdr, bytes([0x78, 0x9C, 0x07, 0, 0, 0, 0])), "block type"),
    }


@pytest.mark.parametrize("case", sorted(_malformed()))
def test_malformed_input_is_an_argument_error(ebo, case):
    data, words = _malformed()[case]
    with pytest.raises(ebo.EboError) as e:
        ebo.decode_png8(data)
    assert e.value.code == ebo.ERR_ARG, str(e.value)
    assert words in str(e.value), str(e.value)


def test_ancillary_chunks_are_skipped_even_when_broken(ebo):
    img = _image(np.random.default_rng(9), 5, 8)
    ihdr = struct.pack(">IIBBBBB", 8, 5, 8, 0, 0, 0, 0)
    broken = bytearray(_chunk(b"tEXt", b"Comment\x00hello"))
    broken[-1] ^= 0xFF  # its CRC
    assert np.array_equal(ebo.decode_png8(_png(ihdr, zlib.compress(_raw_rows(img)), extra=bytes(broken))), img)


def _fuzz_cases(synth):
    """A small PNG, and a seeded sample of (offset, xor) byte flips over all of it."""
    img = _image(np.random.default_rng(11), 5, 9)
    png = synth.png8_bytes(img, filters=4)
    rng = np.random.default_rng(20261016)
    offs = rng.integers(0, len(png), size=600)
    xors = rng.integers(1, 256, size=600)
    return img, png, list(zip(offs.tolist(), xors.tolist()))


def test_every_truncation_and_byte_flip_is_refused(ebo, synth):
    img, png, flips = _fuzz_cases(synth)
    assert np.array_equal(ebo.decode_png8(png), img)
    for n in range(len(png)):
        with pytest.raises(ebo.EboError) as e:
            ebo.decode_png8(png[:n])
        assert e.value.code == ebo.ERR_ARG, (n, str(e.value))
    for off, x in flips:
        b = bytearray(png)
        b[off] ^= x
        with pytest.raises(ebo.EboError) as e:
            ebo.decode_png8(bytes(b))
        assert e.value.code in (ebo.ERR_ARG, ebo.ERR_UNSUPPORTED), (off, x, str(e.value))


def test_fuzz_cases_under_address_sanitizer(synth, tmp_path):
    """The same truncations and flips (plus the golden frames and a round-trip corpus, decoded) through csrc/png8.h
    compiled with -fsanitize=address,undefined: no report."""
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "recording.mk", "OUT=" + str(tmp_path), str(tmp_path / "png8_fuzz")])
    img, png, flips = _fuzz_cases(synth)
    first = tmp_path / "small.png"
    first.write_bytes(png)
    corpus = [str(first)] + list(frontend_ref.FRAMES)
    rng = np.random.default_rng(2)
    for i, (level, strategy, split) in enumerate([(0, None, 1), (6, zlib.Z_FIXED, 100), (9, None, None),
                                                  (1, zlib.Z_RLE, 7), (6, zlib.Z_HUFFMAN_ONLY, None)]):
        p = tmp_path / ("c%d.png" % i)
        p.write_bytes(synth.png8_bytes(_image(rng, 11 + i, 3 + 2 * i), filters=rng.integers(0, 5, size=11 + i),
                                       level=level, strategy=strategy, idat_split=split))
        corpus.append(str(p))
    (tmp_path / "flips.txt").write_text("".join("%d %d\n" % f for f in flips))
    out = subprocess.run([str(tmp_path / "png8_fuzz"), str(tmp_path / "flips.txt")] + corpus, capture_output=True,
                         text=True, timeout=600)
    text = out.stdout + out.stderr
    assert out.returncode == 0, text[-3000:]
    assert "all passed" in out.stdout
    for bad in ("AddressSanitizer", "runtime error", "LeakSanitizer"):
        assert bad not in text, text[-3000:]
