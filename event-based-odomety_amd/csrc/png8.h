// png8.h -- the PNG decoder behind ebo_decode_png8 / ebo_read_png8 and tools::Davis240cRecording: what
// cv::imread(path, CV_8U) returns for a DAVIS frame (an 8-bit greyscale, non-interlaced PNG), without OpenCV, libpng
// or zlib.  Header-only and free of HIP, so that it is built and run on the CPU under AddressSanitizer exactly as it
// ships inside libebo_hip.so (tests/cpp/png8_fuzz.cpp, tests/test_png8_cpu.py).
//
// What it reads (PNG 1.2 / ISO 15948, RFC 1950 / 1951):
//   * the signature, then chunks; the CRC-32 of every critical chunk (IHDR, PLTE, IDAT, IEND) is checked, ancillary
//     chunks are skipped unread (libpng's default on read: a broken ancillary chunk is dropped, not an error);
//   * IHDR: 1 <= width, height <= kMaxSide; bit depth 8 and colour type 0 (grey) only, compression and filter method 0,
//     no interlacing -- any other bit depth, colour type or Adam7 is EBO_ERR_UNSUPPORTED with a message naming it;
//   * the IDAT chunks' concatenation is one zlib stream (CM 8, window <= 32 KB, no preset dictionary -- a dictionary is
//     EBO_ERR_UNSUPPORTED); inflate handles stored, fixed-Huffman and dynamic-Huffman blocks; the stream must hold
//     exactly height * (width + 1) bytes and end in a matching Adler-32;
//   * the five row filters (none, sub, up, average, Paeth) on one byte per pixel.
// Everything malformed -- truncation anywhere, a bad CRC or Adler-32, an invalid Huffman code, a distance behind the
// start of the stream, a stream that ends short of (or runs past) height * (width + 1) bytes, an unknown filter type,
// a missing IEND -- is EBO_ERR_ARG.  No read goes outside the input and no write outside the caller's buffer.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ebo.h"

namespace ebo
{
namespace png
{
constexpr int32_t kMaxSide = 16384;

inline uint32_t crc32(const uint8_t* p, size_t n, uint32_t crc = 0)
{
	static const auto table = [] {
		std::vector<uint32_t> t(256);
		for (uint32_t i = 0; i < 256; ++i)
		{
			uint32_t c = i;
			for (int k = 0; k < 8; ++k)
			{
				c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
			}
			t[i] = c;
		}
		return t;
	}();
	crc = ~crc;
	for (size_t i = 0; i < n; ++i)
	{
		crc = table[(crc ^ p[i]) & 0xFFu] ^ (crc >> 8);
	}
	return ~crc;
}

inline uint32_t adler32(const uint8_t* p, size_t n)
{
	uint32_t a = 1, b = 0;
	while (n)
	{
		const size_t m = n < 5552 ? n : 5552;  // the largest run whose sums cannot overflow 32 bits
		for (size_t i = 0; i < m; ++i)
		{
			a += p[i];
			b += a;
		}
		a %= 65521u;
		b %= 65521u;
		p += m;
		n -= m;
	}
	return (b << 16) | a;
}

inline uint32_t be32(const uint8_t* p)
{
	return (uint32_t(p[0]) << 24) | (uint32_t(p[1]) << 16) | (uint32_t(p[2]) << 8) | uint32_t(p[3]);
}

// ---- inflate (RFC 1951) -------------------------------------------------------------------------------------------
// LSB-first bit reader over [p, p + n); reading past the end is an error, never a read.
struct BitReader
{
	const uint8_t* p;
	size_t n;
	size_t pos = 0;       // next byte to load
	uint64_t buf = 0;     // bits not consumed yet, the oldest in bit 0
	int cnt = 0;          // how many
	bool overrun = false;

	BitReader(const uint8_t* p_, size_t n_) : p(p_), n(n_) {}
	void refill()
	{
		while (cnt <= 56 && pos < n)
		{
			buf |= uint64_t(p[pos++]) << cnt;
			cnt += 8;
		}
	}
	uint32_t bits(int k)  // k <= 24
	{
		if (cnt < k)
		{
			refill();
			if (cnt < k)
			{
				overrun = true;
				return 0;
			}
		}
		const uint32_t v = uint32_t(buf & ((uint64_t(1) << k) - 1));
		buf >>= k;
		cnt -= k;
		return v;
	}
	// to the next byte boundary; the whole bytes still buffered go back to the input
	void align()
	{
		buf >>= (cnt & 7);
		cnt -= (cnt & 7);
		pos -= static_cast<size_t>(cnt / 8);
		buf = 0;
		cnt = 0;
	}
};

// A canonical Huffman code: per length the number of codes, the symbols ordered by (length, value), and a 9-bit
// table for the codes up to 9 bits (entry = symbol << 4 | length, 0 = take the bit-by-bit walk).
struct Huffman
{
	static constexpr int kFast = 9;
	uint16_t count[16];
	uint16_t symbol[288];
	uint16_t fast[1 << kFast];

	// zlib's rules: an over-subscribed set is invalid; an incomplete one only when it is a single code of length 1
	// (or empty) and `allowIncomplete`.  Returns false for an invalid set.
	bool build(const uint8_t* len, int n, bool allowIncomplete)
	{
		std::memset(count, 0, sizeof(count));
		std::memset(fast, 0, sizeof(fast));
		for (int s = 0; s < n; ++s)
		{
			++count[len[s]];
		}
		const int used = n - count[0];
		int left = 1;
		for (int l = 1; l < 16; ++l)
		{
			left <<= 1;
			left -= count[l];
			if (left < 0)
			{
				return false;  // over-subscribed
			}
		}
		if (left > 0 && !(allowIncomplete && used <= 1))
		{
			return false;  // incomplete
		}
		uint16_t offs[16];
		offs[1] = 0;
		for (int l = 1; l < 15; ++l)
		{
			offs[l + 1] = static_cast<uint16_t>(offs[l] + count[l]);
		}
		for (int s = 0; s < n; ++s)
		{
			if (len[s])
			{
				symbol[offs[len[s]]++] = static_cast<uint16_t>(s);
			}
		}
		// the fast table: canonical codes in order of (length, symbol), bit-reversed (deflate sends them MSB first)
		uint32_t code = 0;
		int k = 0;
		for (int l = 1; l <= kFast; ++l)
		{
			for (int c = 0; c < count[l]; ++c, ++k, ++code)
			{
				uint32_t rev = 0;
				for (int b = 0; b < l; ++b)
				{
					rev |= ((code >> b) & 1u) << (l - 1 - b);
				}
				for (uint32_t r = rev; r < (1u << kFast); r += (1u << l))
				{
					fast[r] = static_cast<uint16_t>((symbol[k] << 4) | l);
				}
			}
			code <<= 1;
		}
		return true;
	}

	// the next symbol, or -1 (an unused code, or the input ran out)
	int decode(BitReader& br) const
	{
		if (br.cnt < kFast)
		{
			br.refill();
		}
		const uint16_t e = fast[br.buf & ((1u << kFast) - 1)];
		if (e && (e & 15) <= br.cnt)
		{
			br.buf >>= (e & 15);
			br.cnt -= (e & 15);
			return e >> 4;
		}
		int code = 0, first = 0, index = 0;
		for (int l = 1; l < 16; ++l)
		{
			code |= static_cast<int>(br.bits(1));
			if (br.overrun)
			{
				return -1;
			}
			const int c = count[l];
			if (code - c < first)
			{
				return symbol[index + (code - first)];
			}
			index += c;
			first += c;
			first <<= 1;
			code <<= 1;
		}
		return -1;
	}
};

struct Status
{
	int rc = EBO_OK;
	std::string what;
	bool fail(int code, const std::string& msg)
	{
		rc = code;
		what = msg;
		return false;
	}
};

// Inflates a zlib stream into exactly out.size() bytes (the caller sizes it); false and `st` on any error.
inline bool inflate_zlib(const uint8_t* in, size_t n, std::vector<uint8_t>& out, Status& st)
{
	static const uint16_t lbase[29] = {3,  4,  5,  6,  7,  8,  9,  10, 11,  13,  15,  17,  19,  23, 27,
									   31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
	static const uint8_t lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
	static const uint16_t dbase[30] = {1,   2,   3,   4,   5,   7,    9,    13,   17,   25,   33,   49,   65,    97,    129,
									   193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
	static const uint8_t dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
	static const uint8_t clOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

	if (n < 2)
	{
		return st.fail(EBO_ERR_ARG, "zlib stream truncated (no header)");
	}
	const uint8_t cmf = in[0], flg = in[1];
	if ((cmf & 15) != 8 || (cmf >> 4) > 7 || ((uint32_t(cmf) << 8) | flg) % 31 != 0)
	{
		return st.fail(EBO_ERR_ARG, "bad zlib header (compression method, window size or check bits)");
	}
	if (flg & 0x20)
	{
		return st.fail(EBO_ERR_UNSUPPORTED, "zlib preset dictionary is not supported");
	}
	BitReader br(in + 2, n - 2);
	const size_t cap = out.size();
	size_t o = 0;
	Huffman lit, dist;
	bool last = false;
	while (!last)
	{
		last = br.bits(1) != 0;
		const uint32_t type = br.bits(2);
		if (br.overrun)
		{
			return st.fail(EBO_ERR_ARG, "zlib stream truncated (block header)");
		}
		if (type == 0)
		{
			br.align();
			if (br.n - br.pos < 4)
			{
				return st.fail(EBO_ERR_ARG, "zlib stream truncated (stored block length)");
			}
			const uint8_t* q = br.p + br.pos;
			const uint32_t len = q[0] | (uint32_t(q[1]) << 8), nlen = q[2] | (uint32_t(q[3]) << 8);
			br.pos += 4;
			if (len != (~nlen & 0xFFFFu))
			{
				return st.fail(EBO_ERR_ARG, "stored block length does not match its complement");
			}
			if (br.n - br.pos < len)
			{
				return st.fail(EBO_ERR_ARG, "zlib stream truncated (stored block data)");
			}
			if (cap - o < len)
			{
				return st.fail(EBO_ERR_ARG, "more image data than height * (width + 1) bytes");
			}
			if (len)
			{
				std::memcpy(out.data() + o, br.p + br.pos, len);
			}
			o += len;
			br.pos += len;
			continue;
		}
		if (type == 1)
		{
			uint8_t l[288 + 32];  // (distance codes 30 and 31 complete the fixed code; using them is an error)
			for (int s = 0; s < 144; ++s) l[s] = 8;
			for (int s = 144; s < 256; ++s) l[s] = 9;
			for (int s = 256; s < 280; ++s) l[s] = 7;
			for (int s = 280; s < 288; ++s) l[s] = 8;
			for (int s = 0; s < 32; ++s) l[288 + s] = 5;
			lit.build(l, 288, false);
			dist.build(l + 288, 32, false);
		}
		else if (type == 2)
		{
			const int nlen = static_cast<int>(br.bits(5)) + 257, ndist = static_cast<int>(br.bits(5)) + 1,
					  ncode = static_cast<int>(br.bits(4)) + 4;
			if (br.overrun)
			{
				return st.fail(EBO_ERR_ARG, "zlib stream truncated (dynamic block header)");
			}
			if (nlen > 286 || ndist > 30)
			{
				return st.fail(EBO_ERR_ARG, "dynamic block with too many length or distance codes");
			}
			uint8_t cl[19] = {0};
			for (int i = 0; i < ncode; ++i)
			{
				cl[clOrder[i]] = static_cast<uint8_t>(br.bits(3));
			}
			Huffman clh;
			if (br.overrun)
			{
				return st.fail(EBO_ERR_ARG, "zlib stream truncated (code length code)");
			}
			if (!clh.build(cl, 19, false))
			{
				return st.fail(EBO_ERR_ARG, "invalid code length code");
			}
			uint8_t l[286 + 30] = {0};
			int i = 0;
			while (i < nlen + ndist)
			{
				const int sym = clh.decode(br);
				if (sym < 0)
				{
					return st.fail(EBO_ERR_ARG, br.overrun ? "zlib stream truncated (code lengths)" : "invalid code length symbol");
				}
				if (sym < 16)
				{
					l[i++] = static_cast<uint8_t>(sym);
					continue;
				}
				int rep = 0;
				uint8_t val = 0;
				if (sym == 16)
				{
					if (i == 0)
					{
						return st.fail(EBO_ERR_ARG, "code length repeat with no previous length");
					}
					val = l[i - 1];
					rep = 3 + static_cast<int>(br.bits(2));
				}
				else if (sym == 17)
				{
					rep = 3 + static_cast<int>(br.bits(3));
				}
				else
				{
					rep = 11 + static_cast<int>(br.bits(7));
				}
				if (br.overrun)
				{
					return st.fail(EBO_ERR_ARG, "zlib stream truncated (code lengths)");
				}
				if (i + rep > nlen + ndist)
				{
					return st.fail(EBO_ERR_ARG, "code lengths run past the declared number of codes");
				}
				while (rep--)
				{
					l[i++] = val;
				}
			}
			if (l[256] == 0)
			{
				return st.fail(EBO_ERR_ARG, "dynamic block without an end-of-block code");
			}
			if (!lit.build(l, nlen, true) || !dist.build(l + nlen, ndist, true))
			{
				return st.fail(EBO_ERR_ARG, "invalid literal/length or distance code");
			}
		}
		else
		{
			return st.fail(EBO_ERR_ARG, "invalid deflate block type 3");
		}
		// the Huffman-coded data of a fixed or dynamic block
		for (;;)
		{
			const int sym = lit.decode(br);
			if (sym < 0)
			{
				return st.fail(EBO_ERR_ARG, br.overrun ? "zlib stream truncated (block data)" : "invalid literal/length code");
			}
			if (sym < 256)
			{
				if (o == cap)
				{
					return st.fail(EBO_ERR_ARG, "more image data than height * (width + 1) bytes");
				}
				out[o++] = static_cast<uint8_t>(sym);
				continue;
			}
			if (sym == 256)
			{
				break;
			}
			if (sym > 285)
			{
				return st.fail(EBO_ERR_ARG, "invalid literal/length symbol");
			}
			const size_t len = lbase[sym - 257] + br.bits(lext[sym - 257]);
			const int ds = dist.decode(br);
			if (ds < 0 || ds > 29)
			{
				return st.fail(EBO_ERR_ARG, br.overrun ? "zlib stream truncated (distance)" : "invalid distance code");
			}
			const size_t d = dbase[ds] + br.bits(dext[ds]);
			if (br.overrun)
			{
				return st.fail(EBO_ERR_ARG, "zlib stream truncated (extra bits)");
			}
			if (d > o)
			{
				return st.fail(EBO_ERR_ARG, "distance reaches behind the start of the stream");
			}
			if (cap - o < len)
			{
				return st.fail(EBO_ERR_ARG, "more image data than height * (width + 1) bytes");
			}
			uint8_t* dst = out.data() + o;
			const uint8_t* src = dst - d;
			for (size_t k = 0; k < len; ++k)
			{
				dst[k] = src[k];  // byte by byte: an overlapping copy repeats the run
			}
			o += len;
		}
	}
	if (o != cap)
	{
		return st.fail(EBO_ERR_ARG, "zlib stream ends short of height * (width + 1) bytes");
	}
	br.align();
	if (br.n - br.pos < 4)
	{
		return st.fail(EBO_ERR_ARG, "zlib stream truncated (Adler-32)");
	}
	if (be32(br.p + br.pos) != adler32(out.data(), out.size()))
	{
		return st.fail(EBO_ERR_ARG, "Adler-32 mismatch");
	}
	return true;
}

// ---- PNG ----------------------------------------------------------------------------------------------------------
inline const char* colourTypeName(int ct)
{
	switch (ct)
	{
		case 0: return "greyscale";
		case 2: return "RGB";
		case 3: return "palette";
		case 4: return "greyscale + alpha";
		case 6: return "RGBA";
		default: return "invalid";
	}
}

// The image's size (from IHDR) and, with `pixels`, its [h][w] bytes.  `pixels == nullptr`: IHDR is read and checked
// (signature, CRC, format) and only the size is returned.  EBO_ERR_RANGE (size set) when capacity < w * h.
inline int decode(const uint8_t* in, size_t n, int32_t* w, int32_t* h, uint8_t* pixels, size_t capacity, std::string& err)
{
	static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
	Status st;
	auto fail = [&](int rc, const std::string& what) {
		err = what;
		return rc;
	};
	if (!w || !h || (!in && n))
	{
		return fail(EBO_ERR_ARG, "null argument");
	}
	if (n < 8 || std::memcmp(in, sig, 8) != 0)
	{
		return fail(EBO_ERR_ARG, "not a PNG (signature)");
	}
	size_t pos = 8;
	bool haveHeader = false, haveEnd = false;
	uint32_t width = 0, height = 0;
	std::vector<uint8_t> idat;
	while (!haveEnd)
	{
		if (n - pos < 12)
		{
			return fail(EBO_ERR_ARG, "PNG truncated (chunk header)");
		}
		const uint32_t len = be32(in + pos);
		const uint8_t* type = in + pos + 4;
		if (len > 0x7FFFFFFFu || n - pos - 12 < len)
		{
			return fail(EBO_ERR_ARG, "PNG truncated (chunk data)");
		}
		const uint8_t* data = in + pos + 8;
		const bool critical = !(type[0] & 0x20);
		std::string name(reinterpret_cast<const char*>(type), 4);
		for (char& c : name)
		{
			c = (c >= 32 && c < 127) ? c : '?';  // (messages stay printable; a '?' matches no known chunk)
		}
		pos += 12 + static_cast<size_t>(len);
		if (!haveHeader && name != "IHDR")
		{
			return fail(EBO_ERR_ARG, "PNG does not start with IHDR");
		}
		if (!critical)
		{
			continue;  // ancillary: skipped unread, as libpng does on read
		}
		if (crc32(type, 4 + static_cast<size_t>(len)) != be32(data + len))
		{
			return fail(EBO_ERR_ARG, "CRC-32 mismatch in chunk " + name);
		}
		if (name == "IHDR")
		{
			if (haveHeader || len != 13)
			{
				return fail(EBO_ERR_ARG, "bad IHDR chunk");
			}
			haveHeader = true;
			width = be32(data);
			height = be32(data + 4);
			const int depth = data[8], ct = data[9], comp = data[10], filt = data[11], inter = data[12];
			if (width == 0 || height == 0 || width > uint32_t(kMaxSide) || height > uint32_t(kMaxSide))
			{
				return fail(EBO_ERR_ARG, "image size " + std::to_string(width) + "x" + std::to_string(height) +
											 " outside 1.." + std::to_string(kMaxSide) + " per side");
			}
			if (comp != 0 || filt != 0 || inter > 1)
			{
				return fail(EBO_ERR_ARG, "bad IHDR compression, filter or interlace method");
			}
			if (ct != 0)
			{
				return fail(EBO_ERR_UNSUPPORTED, std::string("colour type ") + std::to_string(ct) + " (" + colourTypeName(ct) +
													 ") is not supported: 8-bit greyscale only");
			}
			if (depth != 8)
			{
				return fail(EBO_ERR_UNSUPPORTED,
							"bit depth " + std::to_string(depth) + " is not supported: 8-bit greyscale only");
			}
			if (inter == 1)
			{
				return fail(EBO_ERR_UNSUPPORTED, "Adam7 interlacing is not supported");
			}
			*w = static_cast<int32_t>(width);
			*h = static_cast<int32_t>(height);
			if (!pixels)
			{
				return EBO_OK;
			}
			if (capacity < size_t(width) * height)
			{
				return fail(EBO_ERR_RANGE, "pixel buffer smaller than width * height");
			}
		}
		else if (name == "IDAT")
		{
			idat.insert(idat.end(), data, data + len);
		}
		else if (name == "IEND")
		{
			haveEnd = true;
		}
		else if (name != "PLTE")  // (a palette is allowed, and unused, in a greyscale image)
		{
			return fail(EBO_ERR_ARG, "unknown critical chunk " + name);
		}
	}
	if (idat.empty())
	{
		return fail(EBO_ERR_ARG, "PNG without image data (IDAT)");
	}
	const size_t stride = size_t(width) + 1;
	std::vector<uint8_t> raw(stride * height);
	if (!inflate_zlib(idat.data(), idat.size(), raw, st))
	{
		return fail(st.rc, st.what);
	}
	// the row filters, one byte per pixel: a = left, b = up, c = up-left (0 outside the image)
	for (uint32_t y = 0; y < height; ++y)
	{
		const uint8_t f = raw[y * stride];
		const uint8_t* line = raw.data() + y * stride + 1;
		uint8_t* cur = pixels + size_t(y) * width;
		const uint8_t* prev = y ? cur - width : nullptr;
		if (f > 4)
		{
			return fail(EBO_ERR_ARG, "unknown row filter type " + std::to_string(f));
		}
		for (uint32_t x = 0; x < width; ++x)
		{
			const int a = x ? cur[x - 1] : 0, b = prev ? prev[x] : 0, c = (prev && x) ? prev[x - 1] : 0;
			int pr = 0;
			switch (f)
			{
				case 0: pr = 0; break;
				case 1: pr = a; break;
				case 2: pr = b; break;
				case 3: pr = (a + b) >> 1; break;
				default:
				{
					const int p = a + b - c, pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
					pr = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
				}
			}
			cur[x] = static_cast<uint8_t>(line[x] + pr);
		}
	}
	return EBO_OK;
}

}  // namespace png
}  // namespace ebo
