// Stand-alone checks of the host IRIS coder (csrc/image_io.cpp encode_iris) and
// of the rule functions the device kernels share with it (csrc/iris_rule.h): no
// GPU, no HIP. Built with the system compiler and -fsanitize=address,undefined
// and run as a child process by tests/test_iris_format.py. Exit status 0 and
// "iris_check: ok" when every check holds; every failed check is printed.
//
// Three things are held against encode_iris's bytes over the shape table (the
// widths 1 .. 513 around the packet cap and the size kernel's step, H = 1 .. 3,
// the three channel counts):
//  - a plain decoder that goes through the two tables, as a reader of the
//    format does, returns the image's row-planes, rows bottom first;
//  - the tables are in the stated order and contiguous, the lengths are the
//    bytes the row-planes take, the file ends with the last one and is within
//    its bound;
//  - the packets that follow from rle_in_run / rle_stretch_start with IrisRle's
//    numbers on windows of eq bits, walked the way the device packer
//    (rle_device.hpp) does a lane at a time (rle_check.h), are the same bytes.
// And over all 256 windows the generic window functions equal the closed form
// of iris_rule.h's comment.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "grey.h"
#include "image_io.hpp"
#include "iris_rule.h"
#include "rle_check.h"

using namespace rr;

static int g_failed = 0, g_checked = 0;

#define CHECK(cond, ...)                                                  \
    do {                                                                  \
        ++g_checked;                                                      \
        if (!(cond)) {                                                    \
            if (++g_failed < 20) {                                        \
                std::printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
                std::printf(__VA_ARGS__);                                 \
                std::printf("\n");                                        \
            }                                                             \
        }                                                                 \
    } while (0)

static uint32_t g_rng = 2463534242u;
static uint32_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 17;
    g_rng ^= g_rng << 5;
    return g_rng;
}

static uint32_t be32(const std::vector<uint8_t>& f, size_t at) {
    return (uint32_t)f[at] << 24 | (uint32_t)f[at + 1] << 16 | (uint32_t)f[at + 2] << 8 | (uint32_t)f[at + 3];
}

// kind 0: random bytes; 1: short runs of a small palette; 2: long runs; 3: one colour.
static std::vector<uint8_t> make_image(int W, int H, int kind) {
    std::vector<uint8_t> img((size_t)W * H * 4);
    int hold = 0;
    uint8_t cur[4] = {9, 9, 9, 255};
    for (size_t i = 0; i < (size_t)W * H; ++i) {
        uint8_t* p = &img[4 * i];
        if (kind == 0) {
            for (int k = 0; k < 4; ++k) p[k] = (uint8_t)rnd();
            continue;
        }
        if (hold == 0 && kind != 3) {
            for (int k = 0; k < 4; ++k) cur[k] = (uint8_t)(60u * (rnd() % 4u));
            hold = kind == 1 ? 1 + (int)(rnd() % 5u) : 1 + (int)(rnd() % 400u);
        }
        --hold;
        std::memcpy(p, cur, 4);
        if (kind != 3 && rnd() % 7u == 0u) p[rnd() % 4u] ^= 0x55;  // a channel of its own
    }
    return img;
}

static void check_image(const std::vector<uint8_t>& img, int W, int H, int C, const char* what) {
    std::vector<uint8_t> file, head;
    CHECK(encode_iris(img.data(), W, H, C, file), "%s %dx%d C=%d refused", what, W, H, C);
    iris_header_bytes(W, H, C, head);
    CHECK(head.size() == kIrisHeaderBytes && file.size() >= head.size() &&
              std::memcmp(file.data(), head.data(), head.size()) == 0,
          "%s %dx%d C=%d header", what, W, H, C);
    CHECK(head[0] == 0x01 && head[1] == 0xDA && head[2] == 1 && head[3] == 1 && head[5] == (C == 1 ? 2 : 3) &&
              head[6] == (W >> 8) && head[7] == (W & 255) && head[8] == (H >> 8) && head[9] == (H & 255) &&
              head[11] == C && head[19] == 255,
          "%s %dx%d C=%d header fields", what, W, H, C);
    const size_t n = (size_t)H * C, body0 = kIrisHeaderBytes;
    CHECK(file.size() - body0 <= iris_body_max_bytes(W, H, C), "%s %dx%d C=%d above the bound", what, W, H, C);
    if (file.size() < body0 + 8 * n) {
        CHECK(false, "%s %dx%d C=%d: no room for the tables", what, W, H, C);
        return;
    }
    size_t expect = body0 + 8 * n;  // where the next coded row-plane starts
    std::vector<uint8_t> again;     // the coded row-planes by the window functions
    for (int f = 0; f < H; ++f)
        for (int z = 0; z < C; ++z) {
            const size_t e = (size_t)f + (size_t)z * H;
            const size_t start = be32(file, body0 + 4 * e), len = be32(file, body0 + 4 * (n + e));
            CHECK(start == expect, "%s %dx%d C=%d row %d channel %d: starts at %zu, not %zu", what, W, H, C, f, z, start,
                  expect);
            if (start != expect || start + len > file.size() || len == 0) {
                CHECK(false, "%s %dx%d C=%d row %d channel %d: table entry outside the file", what, W, H, C, f, z);
                return;
            }
            expect += len;
            std::vector<uint8_t> plane((size_t)W), got;
            for (int x = 0; x < W; ++x) {
                const uint8_t* p = &img[((size_t)(H - 1 - f) * W + (size_t)x) * 4];
                plane[(size_t)x] = C == 1 ? (uint8_t)grey8(p[0], p[1], p[2]) : p[z];
            }
            size_t pos = start;  // the plain decoder: until the count is 0
            bool ok = true;
            while (ok) {
                ok = pos < start + len;
                if (!ok) break;
                const uint8_t b = file[pos++];
                const size_t k = b & 127u;
                if (k == 0) break;
                ok = got.size() + k <= (size_t)W && pos + ((b & 128u) ? k : 1) <= start + len;
                if (!ok) break;
                if (b & 128u) got.insert(got.end(), &file[pos], &file[pos] + k), pos += k;
                else got.insert(got.end(), k, file[pos++]);
            }
            CHECK(ok, "%s %dx%d C=%d row %d channel %d: a packet over the row or its length", what, W, H, C, f, z);
            CHECK(pos == start + len, "%s %dx%d C=%d row %d channel %d: %zu bytes for a length of %zu", what, W, H, C, f, z,
                  pos - start, len);
            CHECK(got == plane, "%s %dx%d C=%d row %d channel %d: decoded bytes differ", what, W, H, C, f, z);
            CHECK(len <= iris_plane_max_bytes((uint64_t)W), "%s %dx%d row %d channel %d: above the row's bound", what, W, H,
                  f, z);
            pack_by_windows<IrisRle>(plane, again);
            again.push_back(0);  // the terminator
        }
    CHECK(expect == file.size(), "%s %dx%d C=%d: %zu trailing bytes", what, W, H, C, file.size() - expect);
    CHECK(again.size() == file.size() - body0 - 8 * n &&
              std::memcmp(again.data(), file.data() + body0 + 8 * n, again.size()) == 0,
          "%s %dx%d C=%d: the window functions give other packets", what, W, H, C);
}

int main() {
    CHECK(window_mismatches<IrisRle>([](auto eq) { return (eq(-1) & eq(0)) | (eq(0) & eq(1)) | (eq(1) & eq(2)); }) == 0,
          "IrisRle: the window functions differ from the closed form");
    const int widths[] = {1, 2, 3, 4, 5, 63, 64, 65, 126, 127, 128, 129, 253, 254, 255, 256, 257, 381, 382, 513};
    const char* names[] = {"random", "short runs", "long runs", "one colour"};
    for (int W : widths)
        for (int H = 1; H <= 3; ++H)
            for (int kind = 0; kind < 4; ++kind) {
                const std::vector<uint8_t> img = make_image(W, H, kind);
                for (int C : {1, 3, 4}) check_image(img, W, H, C, names[kind]);
            }
    // the bound is met: a row of distinct neighbours is all literal
    {
        const int W = 254;
        std::vector<uint8_t> ramp((size_t)W * 4), file;
        for (int x = 0; x < W; ++x)
            for (int k = 0; k < 4; ++k) ramp[4 * (size_t)x + k] = (uint8_t)(x * 3 + k);
        CHECK(encode_iris(ramp.data(), W, 1, 4, file) && file.size() - kIrisHeaderBytes == iris_body_max_bytes(W, 1, 4),
              "an all-literal row is %zu bytes", file.size());
    }
    // the refusals: a side above 65535, a body bound of 2 GB and more, C = 2, no image
    std::vector<uint8_t> out;
    const uint8_t px[4] = {1, 2, 3, 255};
    CHECK(!encode_iris(px, 65536, 1, 4, out) && !encode_iris(px, 1, 65536, 1, out), "a side of 65536");
    CHECK(!encode_iris(px, 65535, 65535, 1, out) && !encode_iris(px, 32768, 16384, 4, out), "a 2 GB bound");
    CHECK(iris_body_max_bytes(65535, 9000, 4) == 0 && iris_body_max_bytes(65535, 9000, 3) != 0, "the bound counts C");
    CHECK(!encode_iris(px, 1, 1, 2, out) && !encode_iris(px, 1, 1, 0, out), "C = 2, 0");
    CHECK(!encode_iris(nullptr, 1, 1, 4, out) && !encode_iris(px, 0, 1, 4, out) && !encode_iris(px, 1, -1, 4, out),
          "no image");
    CHECK(encode_iris(px, 1, 1, 4, out) && out.size() == 512 + 32 + 12 && out[512 + 3] == 32 + 0 && out[512 + 1] == 0,
          "one pixel: %zu bytes", out.size());
    std::printf("iris_check: %s (%d checks, %d failed)\n", g_failed ? "FAILED" : "ok", g_checked, g_failed);
    return g_failed ? 1 : 0;
}
