// png8_fuzz.cpp — csrc/png8.h (the decoder behind ebo_decode_png8) built on its own under AddressSanitizer + UBSan.
//
//   png8_fuzz FLIPS PNG...
// Every PNG must decode; every proper prefix of every PNG (a truncation at each offset) must be refused; and each
// line "<offset> <xor>" of FLIPS, applied to the FIRST PNG, must be refused.  Each case decodes into a buffer of
// exactly w * h bytes on the heap, so that a write past the image is a sanitizer report.  tests/test_png8_cpu.py
// writes the PNGs and FLIPS and runs the same cases through the library.  Prints "all passed".
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../event-based-odomety_amd/csrc/png8.h"

static int g_fail = 0;

static std::vector<uint8_t> readFile(const char* path)
{
	std::vector<uint8_t> out;
	std::FILE* fp = std::fopen(path, "rb");
	if (!fp)
	{
		return out;
	}
	int c;
	while ((c = std::fgetc(fp)) != EOF)
	{
		out.push_back(static_cast<uint8_t>(c));
	}
	std::fclose(fp);
	return out;
}

// decode as the library entry does: the size first, then into a buffer of exactly that size (a copy of the input on
// the heap of exactly n bytes, so that a read past it is reported too)
static int decodeExact(const std::vector<uint8_t>& bytes, size_t n, std::string& err)
{
	std::vector<uint8_t> in(bytes.begin(), bytes.begin() + static_cast<std::ptrdiff_t>(n));
	int32_t w = 0, h = 0;
	int rc = ebo::png::decode(in.data(), in.size(), &w, &h, nullptr, 0, err);
	if (rc != EBO_OK)
	{
		return rc;
	}
	std::vector<uint8_t> px(static_cast<size_t>(w) * h);
	return ebo::png::decode(in.data(), in.size(), &w, &h, px.data(), px.size(), err);
}

int main(int argc, char** argv)
{
	if (argc < 3)
	{
		std::printf("usage: %s FLIPS PNG...\n", argv[0]);
		return 2;
	}
	std::vector<std::vector<uint8_t>> pngs;
	for (int i = 2; i < argc; ++i)
	{
		pngs.push_back(readFile(argv[i]));
		std::string err;
		if (pngs.back().empty() || decodeExact(pngs.back(), pngs.back().size(), err) != EBO_OK)
		{
			std::printf("FAILED: %s does not decode: %s\n", argv[i], err.c_str());
			++g_fail;
		}
	}
	size_t cases = 0;
	for (size_t i = 0; i < pngs.size(); ++i)
	{
		for (size_t n = 0; n < pngs[i].size(); ++n, ++cases)
		{
			std::string err;
			if (decodeExact(pngs[i], n, err) == EBO_OK)
			{
				std::printf("FAILED: %s truncated to %zu bytes decodes\n", argv[2 + i], n);
				++g_fail;
			}
		}
	}
	std::FILE* fp = std::fopen(argv[1], "r");
	if (!fp)
	{
		std::printf("cannot open %s\n", argv[1]);
		return 2;
	}
	unsigned long off = 0, x = 0;
	while (std::fscanf(fp, "%lu %lu", &off, &x) == 2)
	{
		std::vector<uint8_t> b = pngs[0];
		if (off >= b.size())
		{
			continue;
		}
		b[off] ^= static_cast<uint8_t>(x);
		std::string err;
		++cases;
		if (decodeExact(b, b.size(), err) == EBO_OK)
		{
			std::printf("FAILED: flip of byte %lu by 0x%02lx decodes\n", off, x);
			++g_fail;
		}
	}
	std::fclose(fp);
	std::printf("%zu cases\n", cases);
	if (g_fail)
	{
		std::printf("%d FAILED\n", g_fail);
		return 1;
	}
	std::printf("all passed\n");
	return 0;
}
