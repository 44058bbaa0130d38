// Stand-alone checks of the host HDR coder (csrc/image_io.cpp encode_hdr) and
// of the rule functions the device kernels share with it (csrc/hdr_rule.h): no
// GPU, no HIP. Built with the system compiler and -fsanitize=address,undefined
// and run as a child process by tests/test_hdr_format.py. Exit status 0 and
// "hdr_check: ok" when every check holds; every failed check is printed.
//
// Three things are held against encode_hdr's bytes over the shape table (the
// widths 1 .. 257 around the packet caps and the flat / coded thresholds,
// 32767 and 32768, H = 1 .. 3, both channel modes):
//  - a plain decoder of the file returns quads, and they are the quads of an
//    RGBE statement written here with frexp and ldexp in double;
//  - every plane's packets obey the caps, and the file is within its bound;
//  - the packets that follow from rle_in_run / rle_stretch_start with HdrRle's
//    numbers on windows of eq bits, walked the way the device packer
//    (rle_device.hpp) does a lane at a time (rle_check.h), are the same bytes.
// And over all 256 windows the generic window functions equal the closed form
// of hdr_rule.h's comment.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "grey.h"
#include "hdr_rule.h"
#include "image_io.hpp"
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

static uint32_t g_rng = 12345u;
static uint32_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 17;
    g_rng ^= g_rng << 5;
    return g_rng;
}

static float from_bits(uint32_t b) {
    float f;
    std::memcpy(&f, &b, sizeof f);
    return f;
}

// The RGBE rule with frexp and ldexp in double.
static void quad_of(const float* rgb, uint8_t q[4]) {
    double c[3], m = 0.0;
    for (int k = 0; k < 3; ++k) {
        const float v = rgb[k];
        c[k] = (std::isnan(v) || std::signbit(v)) ? 0.0 : std::fmin((double)v, (double)0x1.fep126f);
        m = std::fmax(m, c[k]);
    }
    q[0] = q[1] = q[2] = q[3] = 0;
    if (m < (double)1e-32f) return;
    int e = 0;
    std::frexp(m, &e);
    for (int k = 0; k < 3; ++k) q[k] = (uint8_t)std::floor(std::ldexp(c[k], 8 - e));
    q[3] = (uint8_t)(e + 128);
}

// An image with runs in every plane (a palette with repeats) and noise between.
static std::vector<float> make_image(int W, int H, int kind) {
    static const float pal[6][3] = {{0.f, 0.f, 0.f},          {1.f, 1.f, 1.f},    {0.8f, 0.05f, 0.05f},
                                    {3.5e4f, 2.0e-3f, 7.0f}, {0.18f, 0.18f, 0.18f}, {-1.0f, 0.5f, 2.0e-20f}};
    std::vector<float> img((size_t)W * H * 4);
    int hold = 0, cur = 0;
    for (size_t i = 0; i < (size_t)W * H; ++i) {
        float* p = &img[4 * i];
        if (kind == 2) {  // random bits
            for (int k = 0; k < 4; ++k) p[k] = from_bits(rnd());
            continue;
        }
        if (hold == 0) {
            cur = (int)(rnd() % 6u);
            hold = kind == 0 ? 1 + (int)(rnd() % 9u) : 1 + (int)(rnd() % 400u);
        }
        --hold;
        for (int k = 0; k < 3; ++k) p[k] = pal[cur][k];
        if (rnd() % 5u == 0u) p[rnd() % 3u] = from_bits(0x3F000000u + (rnd() & 0x00FFFFFFu));
        p[3] = from_bits(rnd());  // junk the coder ignores
    }
    return img;
}

static void check_image(const std::vector<float>& img, int W, int H, int C, const char* what) {
    std::vector<uint8_t> file;
    CHECK(encode_hdr(img.data(), W, H, C, file), "%s %dx%d C=%d refused", what, W, H, C);
    const std::string head =
        "#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y " + std::to_string(H) + " +X " + std::to_string(W) + "\n";
    CHECK(file.size() >= head.size() && std::memcmp(file.data(), head.data(), head.size()) == 0, "%s %dx%d header", what,
          W, H);
    CHECK(file.size() - head.size() <= hdr_body_max_bytes(W, H), "%s %dx%d above the bound", what, W, H);
    // the quads the file must hold
    std::vector<uint8_t> want((size_t)W * H * 4);
    for (size_t i = 0; i < (size_t)W * H; ++i) {
        float rgb[3] = {img[4 * i], img[4 * i + 1], img[4 * i + 2]};
        if (C == 1) rgb[0] = rgb[1] = rgb[2] = luma709(rgb[0], rgb[1], rgb[2]);
        quad_of(rgb, &want[4 * i]);
    }
    size_t pos = head.size();
    std::vector<uint8_t> again;  // the body by the window functions
    bool ok = true;
    for (int y = 0; y < H && ok; ++y) {
        const uint8_t* wq = &want[(size_t)y * W * 4];
        if (hdr_row_flat(W)) {
            ok = pos + 4 * (size_t)W <= file.size() && std::memcmp(&file[pos], wq, 4 * (size_t)W) == 0;
            CHECK(ok, "%s %dx%d C=%d row %d: flat quads differ", what, W, H, C, y);
            pos += 4 * (size_t)W;
            continue;
        }
        const uint8_t marker[4] = {2, 2, (uint8_t)(W >> 8), (uint8_t)W};
        ok = pos + 4 <= file.size() && std::memcmp(&file[pos], marker, 4) == 0;
        CHECK(ok, "%s %dx%d row %d: marker", what, W, H, y);
        pos += 4;
        again.insert(again.end(), marker, marker + 4);
        for (int k = 0; k < 4 && ok; ++k) {
            std::vector<uint8_t> plane((size_t)W), got;
            for (int x = 0; x < W; ++x) plane[(size_t)x] = wq[4 * (size_t)x + k];
            while (got.size() < (size_t)W && ok) {  // the plain decoder
                ok = pos < file.size();
                if (!ok) break;
                const uint8_t b = file[pos++];
                const bool run = b > 128;
                const size_t n = run ? b - 128u : b;
                ok = n >= 1 && got.size() + n <= (size_t)W && pos + (run ? 1 : n) <= file.size();
                if (!ok) break;
                if (run) got.insert(got.end(), n, file[pos++]);
                else got.insert(got.end(), &file[pos], &file[pos] + n), pos += n;
            }
            CHECK(ok, "%s %dx%d C=%d row %d plane %d: a packet of count 0, over the plane or the file", what, W, H, C, y, k);
            CHECK(got == plane, "%s %dx%d C=%d row %d plane %d: decoded bytes differ", what, W, H, C, y, k);
            pack_by_windows<HdrRle>(plane, again);
        }
    }
    CHECK(!ok || pos == file.size(), "%s %dx%d: %zu trailing bytes", what, W, H, file.size() - pos);
    if (ok && !hdr_row_flat(W))
        CHECK(again.size() == file.size() - head.size() &&
                  std::memcmp(again.data(), file.data() + head.size(), again.size()) == 0,
              "%s %dx%d C=%d: the window functions give other packets", what, W, H, C);
}

int main() {
    // the four windows of three consecutive eq bits that cover the byte
    CHECK(window_mismatches<HdrRle>([](auto eq) {
              return (eq(-2) & eq(-1) & eq(0)) | (eq(-1) & eq(0) & eq(1)) | (eq(0) & eq(1) & eq(2)) |
                     (eq(1) & eq(2) & eq(3));
          }) == 0,
          "HdrRle: the window functions differ from the closed form");
    const int widths[] = {1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513, 32767, 32768};
    for (int W : widths)
        for (int H = 1; H <= 3; ++H) {
            if (W > 1000 && H != 2) continue;
            for (int kind = 0; kind < 3; ++kind) {
                const std::vector<float> img = make_image(W, H, kind);
                const char* what = kind == 0 ? "short runs" : kind == 1 ? "long runs" : "random bits";
                check_image(img, W, H, 3, what);
                check_image(img, W, H, 1, what);
            }
        }
    // planes that are one run, and one literal stretch
    for (int W : {8, 126, 127, 128, 129, 254, 255, 256, 381, 382}) {
        std::vector<float> flat((size_t)W * 4, 0.25f), ramp((size_t)W * 4);
        for (int x = 0; x < W; ++x)
            for (int k = 0; k < 4; ++k) ramp[4 * (size_t)x + k] = std::ldexp(1.0f + (float)((x * 37 + k) % 128) / 128.0f, x % 5);
        check_image(flat, W, 1, 3, "one run");
        check_image(ramp, W, 1, 3, "ramp");
    }
    // the refusals: a body bound of 2 GB and more, a channel count that is not 1 or 3, no image
    std::vector<uint8_t> out;
    const float px[4] = {1.f, 1.f, 1.f, 1.f};
    CHECK(!encode_hdr(px, 32768, 16384, 3, out), "a 2 GB flat body");
    CHECK(!encode_hdr(px, 32767, 16400, 3, out), "a coded bound above 2 GB");
    CHECK(!encode_hdr(px, 1, 1, 4, out) && !encode_hdr(px, 1, 1, 2, out), "C = 4, 2");
    CHECK(!encode_hdr(nullptr, 1, 1, 3, out) && !encode_hdr(px, 0, 1, 3, out) && !encode_hdr(px, 1, -1, 3, out), "no image");
    CHECK(encode_hdr(px, 1, 1, 3, out) && out.size() >= 4 && out[out.size() - 4] == 128 && out.back() == 129, "1.0");
    std::printf("hdr_check: %s (%d checks, %d failed)\n", g_failed ? "FAILED" : "ok", g_checked, g_failed);
    return g_failed ? 1 : 0;
}
