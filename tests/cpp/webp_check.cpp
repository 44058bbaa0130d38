// Stand-alone checks of the host WEBP coder (csrc/image_io.cpp encode_webp) and
// of the rule functions the device kernels share with it (csrc/webp_rule.h): no
// GPU, no HIP. Built with the system compiler and -fsanitize=address,undefined
// and run as a child process by tests/test_webp_format.py. Exit status 0 and
// "webp_check: ok" when every check holds; every failed check is printed.
//
// Three things are held against encode_webp's bytes over the shape table
// (widths around the size kernel's step and the copy limit, H = 1 .. 3, the
// three colour modes, four kinds of content):
//  - the container's sizes, the pad byte, and the payload within its bound;
//  - a plain decoder of the subset (two transforms, five prefix codes, copies at
//    distance code 2) returns the image's pixels and ends on the payload's last
//    byte;
//  - the tokens that follow from webp_kind on windows of eq bits, taken a pixel
//    at a time the way webp.hip k_webp_size takes a lane, are the decoder's.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "grey.h"
#include "image_io.hpp"
#include "webp_rule.h"

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

// kind 0: random bytes; 1: runs of random lengths of a small palette; 2: one colour; 3: a ramp.
static std::vector<uint8_t> make_image(int W, int H, int kind) {
    std::vector<uint8_t> img((size_t)W * H * 4);
    int hold = 0;
    uint8_t cur[4] = {9, 9, 9, 255};
    for (size_t i = 0; i < (size_t)W * H; ++i) {
        if (kind == 0 || (kind == 1 && hold-- <= 0)) {
            for (int k = 0; k < 4; ++k) cur[k] = kind == 0 ? (uint8_t)rnd() : (uint8_t)(40 * (rnd() % 3) + k);
            hold = (int)(rnd() % 7);
        }
        if (kind == 3)
            for (int k = 0; k < 4; ++k) cur[k] = (uint8_t)((i % (size_t)W) * (size_t)(k + 1));
        std::memcpy(&img[4 * i], cur, 4);
    }
    return img;
}

struct BitsIn {
    const uint8_t* d;
    size_t n, pos = 0;
    bool bad = false;
    uint32_t get(int nb) {
        uint32_t v = 0;
        for (int k = 0; k < nb; ++k, ++pos) {
            if (pos / 8 >= n) {
                bad = true;
                return 0;
            }
            v |= (uint32_t)((d[pos / 8] >> (pos % 8)) & 1u) << k;
        }
        return v;
    }
};

// A prefix code as its lengths; reading walks the canonical code a bit at a time.
struct Code {
    std::vector<int> lens;
    int only = -1;  // its one used symbol: no bits
    bool complete = true;
    void finish() {
        int used = 0;
        uint64_t kraft = 0;
        for (size_t s = 0; s < lens.size(); ++s)
            if (lens[s]) ++used, only = (int)s, kraft += 1ull << (15 - lens[s]);
        if (used != 1) only = -1, complete = kraft == 1ull << 15;
    }
    int read(BitsIn& in) const {
        if (only >= 0) return only;
        uint32_t code = 0, first = 0;
        for (int l = 1; l <= 15; ++l) {
            code = code << 1 | in.get(1);
            uint32_t count = 0;
            for (int v : lens) count += v == l;
            if (code - first < count) {
                uint32_t k = code - first;
                for (size_t s = 0; s < lens.size(); ++s)
                    if (lens[s] == l && k-- == 0) return (int)s;
            }
            first = (first + count) << 1;
        }
        in.bad = true;
        return 0;
    }
};

static Code read_code(BitsIn& in, int n) {
    Code c;
    c.lens.assign((size_t)n, 0);
    if (in.get(1)) {
        const int k = (int)in.get(1) + 1;
        const uint32_t s0 = in.get(in.get(1) ? 8 : 1);
        c.lens[s0] = 1;
        if (k == 2) c.lens[in.get(8)] = 1;
    } else {
        Code cl;
        cl.lens.assign(19, 0);
        const int num = 4 + (int)in.get(4);
        for (int k = 0; k < num; ++k) cl.lens[(size_t)webp_cl_order(k)] = (int)in.get(3);
        cl.finish();
        if (in.get(1) || !cl.complete) in.bad = true;  // max_symbol is not written by this project
        for (int s = 0; s < n && !in.bad; ++s) {
            const int l = cl.read(in);
            if (l > 15) in.bad = true;  // nor are the repeat codes
            else c.lens[(size_t)s] = l;
        }
    }
    c.finish();
    if (!c.complete) in.bad = true;
    return c;
}

static uint32_t unprefix(BitsIn& in, uint32_t p) {
    if (p < 4) return p + 1;
    const uint32_t extra = (p - 2) >> 1;
    return ((2 + (p & 1)) << extra) + in.get((int)extra) + 1;
}

// token: 0 for a literal, else a copy's length
static bool decode(const std::vector<uint8_t>& file, int W, int H, int C, std::vector<uint32_t>& resid,
                   std::vector<uint32_t>& tokens) {
    if (file.size() < kWebpRiffBytes) return false;
    uint32_t n;
    std::memcpy(&n, &file[16], 4);
    BitsIn in{file.data() + kWebpRiffBytes, n};
    bool ok = in.get(8) == 0x2F && (int)in.get(14) == W - 1 && (int)in.get(14) == H - 1;
    ok = ok && in.get(1) == (C == 4 ? 1u : 0u) && in.get(3) == 0;
    ok = ok && in.get(1) == 1 && in.get(2) == 2 && in.get(1) == 1 && in.get(2) == 0;
    ok = ok && in.get(3) + 2 == kWebpBlockBits && in.get(1) == 0;
    if (!ok) return false;
    for (int a = 0; a < kWebpAlphabets; ++a) {
        const Code c = read_code(in, webp_size(a));
        if (c.only != (a == 0 ? 1 : 0)) return false;  // mode 1; the blocks take no bits
    }
    if (in.get(1) || in.get(1) || in.get(1)) return false;
    Code code[kWebpAlphabets];
    for (int a = 0; a < kWebpAlphabets; ++a) code[a] = read_code(in, webp_size(a));
    resid.assign((size_t)W * H, 0);
    tokens.clear();
    for (int y = 0; y < H && !in.bad; ++y)
        for (int x = 0; x < W && !in.bad;) {
            uint32_t* row = &resid[(size_t)y * W];
            const uint32_t g = (uint32_t)code[0].read(in);
            if (g < 256) {
                const uint32_t r = (uint32_t)code[1].read(in), b = (uint32_t)code[2].read(in);
                row[x++] = (uint32_t)code[3].read(in) << 24 | r << 16 | g << 8 | b;
                tokens.push_back(0);
                continue;
            }
            const uint32_t len = unprefix(in, g - 256);
            if (unprefix(in, (uint32_t)code[4].read(in)) != 2 || x == 0 || x + (int)len > W) return false;
            for (uint32_t k = 0; k < len; ++k, ++x) row[x] = row[x - 1];
            tokens.push_back(len);
        }
    return !in.bad && (in.pos + 7) / 8 == n;
}

static void check_shape(int W, int H, int C, int kind) {
    const std::vector<uint8_t> img = make_image(W, H, kind);
    std::vector<uint8_t> file;
    CHECK(encode_webp(img.data(), W, H, C, file), "%dx%d C%d", W, H, C);
    uint32_t riff, n;
    std::memcpy(&riff, &file[4], 4);
    std::memcpy(&n, &file[16], 4);
    CHECK(std::memcmp(&file[0], "RIFF", 4) == 0 && std::memcmp(&file[8], "WEBPVP8L", 8) == 0, "%dx%d", W, H);
    CHECK(riff == file.size() - 8 && file.size() == kWebpRiffBytes + n + (n & 1u), "%dx%d sizes", W, H);
    CHECK(!(n & 1u) || file.back() == 0, "%dx%d pad", W, H);
    CHECK(n <= webp_body_max_bytes(W, H, C), "%dx%d bound", W, H);
    std::vector<uint32_t> resid, tokens;
    CHECK(decode(file, W, H, C, resid, tokens), "%dx%d C%d kind %d decode", W, H, C, kind);
    if (resid.size() != (size_t)W * H) return;
    // the residuals are the image's
    auto pixel = [&](size_t i) {
        uint32_t v;
        std::memcpy(&v, &img[4 * i], 4);
        return webp_pixel(v, C);
    };
    size_t wrong = 0;
    for (size_t i = 0; i < (size_t)W * H; ++i) {
        const uint32_t pred = i % (size_t)W ? pixel(i - 1) : i ? pixel(i - (size_t)W) : kWebpFirstPrediction;
        wrong += webp_sub(pixel(i), pred) != resid[i];
    }
    CHECK(wrong == 0, "%dx%d C%d kind %d: %zu residuals differ", W, H, C, kind, wrong);
    // the tokens of webp_kind, a pixel at a time
    std::vector<uint32_t> mine;
    for (int y = 0; y < H; ++y) {
        const uint32_t* row = &resid[(size_t)y * W];
        auto eq = [&](int j) { return j > 0 && j < W && row[j] == row[j - 1]; };
        int first = 0;
        for (int i = 0; i < W; ++i) {
            uint32_t win = 0;
            for (uint32_t k = 0; k < kWebpMinRun; ++k) win |= (eq(i + (int)k) ? 1u : 0u) << k;
            if (eq(i) && !eq(i - 1)) first = i;
            const uint32_t q = eq(i) ? (uint32_t)(i - first) : 0u;
            const int kind_i = webp_kind(win, q);
            if (kind_i == kWebpLiteral) mine.push_back(0);
            if (kind_i == kWebpCopy) {  // its length: to the chunk's end
                int e = i;
                while (eq(e + 1) && (uint32_t)(e + 1 - first) % kWebpMaxCopy != 0) ++e;
                mine.push_back((uint32_t)(e - i + 1));
            }
        }
    }
    CHECK(mine == tokens, "%dx%d C%d kind %d: %zu tokens by webp_kind, %zu in the file", W, H, C, kind, mine.size(),
          tokens.size());
}

int main() {
    uint32_t sym, nb, extra;
    webp_prefix(1, sym, nb, extra);
    CHECK(sym == 0 && nb == 0, "prefix(1)");
    webp_prefix(2, sym, nb, extra);
    CHECK(sym == kWebpDistSym && nb == 0, "prefix(2)");
    webp_prefix(4096, sym, nb, extra);
    CHECK(sym == 23 && nb == 10 && extra == 1023, "prefix(4096)");
    for (uint32_t v = 1; v <= 4096; ++v) {  // every length comes back
        webp_prefix(v, sym, nb, extra);
        const uint32_t back = sym < 4 ? sym + 1 : ((2 + (sym & 1)) << ((sym - 2) >> 1)) + extra + 1;
        CHECK(back == v && sym < 24 && (sym < 4 ? nb == 0 : nb == (sym - 2) >> 1), "prefix(%u)", v);
    }
    CHECK(webp_sub(0x01020304u, 0x04030201u) == 0xFDFF0103u, "sub");
    CHECK(webp_pixel(0x80402010u, 4) == (0x80u << 24 | 0xF0u << 16 | 0x20u << 8 | 0x20u), "pixel RGBA");
    CHECK(webp_pixel(0x80402010u, 3) >> 24 == 255, "pixel RGB");
    CHECK(webp_pixel(0x80402010u, 1) == (0xFF000000u | grey8(0x10, 0x20, 0x40) << 8), "pixel BW");
    CHECK(webp_body_max_bytes(16385, 1, 4) == 0 && webp_body_max_bytes(1, 16385, 4) == 0, "side");
    // the largest image's bound stays below 2 GB: the side limit is the only size refusal
    CHECK(webp_body_max_bytes(16384, 16384, 4) == (kWebpHeaderMaxBits + 60ull * 16384 * 16384 + 7) / 8, "largest");
    CHECK(webp_body_max_bytes(16384, 16384, 4) < (1ull << 31), "below 2 GB");
    CHECK(webp_body_max_bytes(1, 1, 2) == 0 && webp_body_max_bytes(0, 1, 4) == 0, "mode");
    CHECK(webp_body_max_bytes(16384, 1, 4) != 0, "16384 is inside");
    const int widths[] = {1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 300, 513, 4097, 4100, 8195};
    for (int W : widths)
        for (int H = 1; H <= (W > 600 ? 1 : 3); ++H)
            for (int C : {1, 3, 4})
                for (int kind = 0; kind < 4; ++kind) check_shape(W, H, C, kind);
    check_shape(16384, 1, 4, 2);
    check_shape(40, 300, 4, 1);
    std::vector<uint8_t> out;
    uint8_t px[4] = {1, 2, 3, 4};
    CHECK(!encode_webp(nullptr, 1, 1, 4, out) && !encode_webp(px, 16385, 1, 4, out) && !encode_webp(px, 1, 1, 2, out),
          "refusals");
    std::printf("webp_check: %d checks, %d failed\n", g_checked, g_failed);
    if (g_failed) return 1;
    std::printf("webp_check: ok\n");
    return 0;
}
