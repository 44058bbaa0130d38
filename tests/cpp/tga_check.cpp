// Stand-alone checks of the host TARGA coder (csrc/image_io.cpp encode_tga) and
// of the rule functions the device packer shares with it (csrc/tga_rule.h,
// csrc/rle_rule.h): no GPU, no HIP. Built with the system compiler and
// -fsanitize=address,undefined and run as a child process by
// tests/test_tga_format.py. Exit status 0 and "tga_check: ok" when every check
// holds; every failed check is printed.
//
// Held against encode_tga's bytes over the shape table (the widths 1 .. 513
// around the packet cap and the packer's step, H = 1 .. 3, the three channel
// counts):
//  - a plain decoder of the packets returns the image's pixels, rows bottom
//    first, no packet crosses a row, and the file is within its bound;
//  - the packets that follow from rle_in_run / rle_stretch_start with
//    TgaRle<C>'s numbers on windows of eq bits, walked the way the device
//    packer (rle_device.hpp) does a lane at a time (rle_check.h), are the same
//    bytes.
// Over all 256 windows the generic window functions equal the closed forms of
// tga_rule.h's comment, and an all-literal row meets the bound.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "grey.h"
#include "image_io.hpp"
#include "rle_check.h"
#include "tga_rule.h"

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

template <int C>
static void check_image(const std::vector<uint8_t>& img, int W, int H, const char* what) {
    std::vector<uint8_t> file, head;
    CHECK(encode_tga(img.data(), W, H, C, true, file), "%s %dx%d C=%d refused", what, W, H, C);
    tga_header_bytes(W, H, C, true, head);
    CHECK(head.size() == kTgaHeaderBytes && file.size() >= head.size() &&
              std::memcmp(file.data(), head.data(), head.size()) == 0,
          "%s %dx%d C=%d header", what, W, H, C);
    CHECK(file.size() - head.size() <= tga_body_max_bytes(W, H, C, true), "%s %dx%d C=%d above the bound", what, W, H, C);
    size_t pos = head.size();
    std::vector<uint8_t> again;  // the body by the window functions
    bool ok = true;
    for (int f = 0; f < H && ok; ++f) {  // file row f: bottom row first
        std::vector<uint8_t> row((size_t)W * C), got;
        for (int x = 0; x < W; ++x) {
            const uint8_t* p = &img[((size_t)(H - 1 - f) * W + (size_t)x) * 4];
            uint8_t* q = &row[(size_t)x * C];
            if (C == 1) {
                q[0] = (uint8_t)grey8(p[0], p[1], p[2]);
            } else {
                q[0] = p[2], q[1] = p[1], q[2] = p[0];
                if (C == 4) q[3] = p[3];
            }
        }
        const size_t row_at = pos;
        while (got.size() < row.size() && ok) {  // the plain decoder
            ok = pos < file.size();
            if (!ok) break;
            const uint8_t b = file[pos++];
            const bool run = (b & 128u) != 0u;
            const size_t n = (b & 127u) + 1u;
            ok = got.size() + n * C <= row.size() && pos + (run ? 1 : n) * C <= file.size();
            if (!ok) break;
            if (run) {
                for (size_t k = 0; k < n; ++k) got.insert(got.end(), &file[pos], &file[pos] + C);
                pos += C;
            } else {
                got.insert(got.end(), &file[pos], &file[pos] + n * C), pos += n * C;
            }
        }
        CHECK(ok, "%s %dx%d C=%d row %d: a packet over the row or the file", what, W, H, C, f);
        CHECK(got == row, "%s %dx%d C=%d row %d: decoded pixels differ", what, W, H, C, f);
        CHECK(pos - row_at <= tga_row_max_bytes((uint64_t)W, (uint64_t)C), "%s %dx%d C=%d row %d: above the row's bound",
              what, W, H, C, f);
        pack_by_windows<TgaRle<C>>(row, again);
    }
    CHECK(!ok || pos == file.size(), "%s %dx%d C=%d: %zu trailing bytes", what, W, H, C, file.size() - pos);
    CHECK(again.size() == file.size() - head.size() &&
              std::memcmp(again.data(), file.data() + head.size(), again.size()) == 0,
          "%s %dx%d C=%d: the window functions give other packets", what, W, H, C);
}

int main() {
    // C = 3, 4: a run from two equal pixels; C = 1: from three
    auto two = [](auto eq) { return eq(0) | eq(1); };
    auto three = [](auto eq) { return (eq(-1) & eq(0)) | (eq(0) & eq(1)) | (eq(1) & eq(2)); };
    CHECK(window_mismatches<TgaRle<4>>(two) == 0, "TgaRle<4>: the window functions differ from the closed form");
    CHECK(window_mismatches<TgaRle<3>>(two) == 0, "TgaRle<3>: the window functions differ from the closed form");
    CHECK(window_mismatches<TgaRle<1>>(three) == 0, "TgaRle<1>: the window functions differ from the closed form");
    const int widths[] = {1, 2, 3, 4, 5, 63, 64, 65, 126, 127, 128, 129, 253, 254, 255, 256, 257, 381, 382, 513};
    const char* names[] = {"random", "short runs", "long runs", "one colour"};
    for (int W : widths)
        for (int H = 1; H <= 3; ++H)
            for (int kind = 0; kind < 4; ++kind) {
                const std::vector<uint8_t> img = make_image(W, H, kind);
                check_image<1>(img, W, H, names[kind]);
                check_image<3>(img, W, H, names[kind]);
                check_image<4>(img, W, H, names[kind]);
            }
    // the bound is met: a row of distinct neighbours is all literal
    {
        const int W = 257;
        std::vector<uint8_t> ramp((size_t)W * 4), file;
        for (int x = 0; x < W; ++x)
            for (int k = 0; k < 4; ++k) ramp[4 * (size_t)x + k] = (uint8_t)(x * 3 + k);
        for (int C : {1, 3, 4})
            CHECK(encode_tga(ramp.data(), W, 1, C, true, file) &&
                      file.size() - kTgaHeaderBytes == tga_body_max_bytes(W, 1, C, true),
                  "an all-literal row of C=%d is %zu bytes", C, file.size());
    }
    std::printf("tga_check: %s (%d checks, %d failed)\n", g_failed ? "FAILED" : "ok", g_checked, g_failed);
    return g_failed ? 1 : 0;
}
