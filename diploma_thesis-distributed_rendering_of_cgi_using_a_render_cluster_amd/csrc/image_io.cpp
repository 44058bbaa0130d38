// Host image encoders: baseline JPEG (JFIF, 4:2:0, ITU T.81 Annex K tables,
// IJG quality scaling) and PNG (zlib). Replaces Blender's write_still for the
// formats the reference jobs use: "JPEG" with quality forced to 90
// (/root/reference/scripts/render-timing-script.py:83-84) and "PNG"
// (blender-projects/02_physics/02-physics_demo_170f-5w_naive-fine.toml:13).
//
// The JPEG entropy coder runs one restart interval per MCU row, so rows are
// encoded on parallel host threads and joined with RSTn markers.
#include "image_io.hpp"

#include "exr_rle_rule.h"
#include "grey.h"
#include "hdr_rule.h"
#include "iris_rule.h"
#include "png_filter.h"
#include "tga_rule.h"
#include "webp_rule.h"

#include <zlib.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <thread>

#include <sched.h>

namespace rr {

// Host threads of the encoders: the CPUs this process may run on (a worker
// pinned to its GPU's NUMA node — bench.py gpu_placement — gets that share,
// not the machine's count), at most 16.
int encoder_threads() {
    int n = 0;
    cpu_set_t set;
    CPU_ZERO(&set);
    if (sched_getaffinity(0, sizeof set, &set) == 0) n = CPU_COUNT(&set);
    if (n <= 0) n = (int)std::thread::hardware_concurrency();
    if (n <= 0) n = 4;
    return std::min(n, 16);
}

namespace {

// ---------------------------------------------------------------- JPEG ----
const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                             12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                             35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                             58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

const uint8_t kStdLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                              14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                              18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                              49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint8_t kStdChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99,
                                24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// Annex K.3 Huffman tables: BITS (16) + HUFFVAL.
const uint8_t kDcLumBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const uint8_t kDcLumVal[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kDcChrBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
const uint8_t kDcChrVal[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kAcLumBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
const uint8_t kAcLumVal[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
    0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
    0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
const uint8_t kAcChrBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
const uint8_t kAcChrVal[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
    0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
    0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
    0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
    0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

struct HuffTable {
    uint16_t code[256];
    uint8_t len[256];
    void build(const uint8_t bits[16], const uint8_t* vals) {
        std::memset(len, 0, sizeof len);
        uint16_t c = 0;
        int k = 0;
        for (int l = 1; l <= 16; ++l) {
            for (int i = 0; i < bits[l - 1]; ++i) {
                code[vals[k]] = c++;
                len[vals[k]] = (uint8_t)l;
                ++k;
            }
            c <<= 1;
        }
    }
};

struct Tables {
    HuffTable dc[2], ac[2];
    Tables() {
        dc[0].build(kDcLumBits, kDcLumVal);
        dc[1].build(kDcChrBits, kDcChrVal);
        ac[0].build(kAcLumBits, kAcLumVal);
        ac[1].build(kAcChrBits, kAcChrVal);
    }
};
const Tables& tables() {
    static Tables t;
    return t;
}

struct BitWriter {
    std::vector<uint8_t>& out;
    uint32_t acc = 0;
    int nbits = 0;
    explicit BitWriter(std::vector<uint8_t>& o) : out(o) {}
    inline void put(uint32_t code, int len) {
        acc = (acc << len) | (code & ((1u << len) - 1u));
        nbits += len;
        while (nbits >= 8) {
            const uint8_t b = (uint8_t)(acc >> (nbits - 8));
            out.push_back(b);
            if (b == 0xFF) out.push_back(0x00);
            nbits -= 8;
        }
        acc &= (1u << nbits) - 1u;
    }
    void flush() {  // pad with 1-bits
        if (nbits > 0) put((1u << (8 - nbits)) - 1u, 8 - nbits);
    }
};

// IJG jpeg_quality_scaling + jpeg_add_quant_table (force_baseline).
void quant_table(const uint8_t* base, int quality, uint8_t* q) {
    quality = std::min(std::max(quality, 1), 100);
    const int scale = quality < 50 ? 5000 / quality : 200 - quality * 2;
    for (int i = 0; i < 64; ++i) {
        long t = ((long)base[i] * scale + 50L) / 100L;
        if (t <= 0) t = 1;
        if (t > 255) t = 255;
        q[i] = (uint8_t)t;
    }
}

struct Dct {
    float c[8][8];  // c[u][x] = C(u)/2 cos((2x+1) u pi / 16)
    Dct() {
        for (int u = 0; u < 8; ++u)
            for (int x = 0; x < 8; ++x)
                c[u][x] = (float)((u == 0 ? std::sqrt(0.5) : 1.0) * 0.5 * std::cos((2 * x + 1) * u * M_PI / 16.0));
    }
};
const Dct& dct() {
    static Dct d;
    return d;
}

// Forward DCT + quantisation of one 8x8 block (level-shifted samples).
void fdct_quant(const float in[64], const float qinv[64], int16_t* out) {
    const Dct& D = dct();
    float tmp[64];
    for (int y = 0; y < 8; ++y)
        for (int u = 0; u < 8; ++u) {
            float s = 0.f;
            for (int x = 0; x < 8; ++x) s += D.c[u][x] * in[8 * y + x];
            tmp[8 * y + u] = s;
        }
    for (int v = 0; v < 8; ++v)
        for (int u = 0; u < 8; ++u) {
            float s = 0.f;
            for (int y = 0; y < 8; ++y) s += D.c[v][y] * tmp[8 * y + u];
            out[8 * v + u] = (int16_t)std::lrint(s * qinv[8 * v + u]);
        }
}

inline int bitlen(int v) {
    v = v < 0 ? -v : v;
    int n = 0;
    while (v) { ++n; v >>= 1; }
    return n;
}

void encode_block(BitWriter& bw, const int16_t* blk, int& pred, const HuffTable& dc, const HuffTable& ac) {
    const int diff = blk[0] - pred;
    pred = blk[0];
    int n = bitlen(diff);
    bw.put(dc.code[n], dc.len[n]);
    if (n) bw.put(diff < 0 ? (uint32_t)(diff - 1) : (uint32_t)diff, n);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = blk[kZigzag[k]];
        if (v == 0) {
            ++run;
            continue;
        }
        while (run > 15) {
            bw.put(ac.code[0xF0], ac.len[0xF0]);
            run -= 16;
        }
        n = bitlen(v);
        const int sym = (run << 4) | n;
        bw.put(ac.code[sym], ac.len[sym]);
        bw.put(v < 0 ? (uint32_t)(v - 1) : (uint32_t)v, n);
        run = 0;
    }
    if (run) bw.put(ac.code[0x00], ac.len[0x00]);
}

void put16(std::vector<uint8_t>& o, int v) {
    o.push_back((uint8_t)(v >> 8));
    o.push_back((uint8_t)v);
}

void write_dht(std::vector<uint8_t>& o, int cls, int id, const uint8_t bits[16], const uint8_t* vals) {
    int n = 0;
    for (int i = 0; i < 16; ++i) n += bits[i];
    o.push_back(0xFF); o.push_back(0xC4);
    put16(o, 2 + 1 + 16 + n);
    o.push_back((uint8_t)((cls << 4) | id));
    o.insert(o.end(), bits, bits + 16);
    o.insert(o.end(), vals, vals + n);
}

// Forward DCT + quantisation of MCU row `my` (16 pixel rows) on the host:
// coefficients [mcux][6][64] (blocks Y00 Y01 Y10 Y11 Cb Cr, natural order).
// jpeg.hip computes the same values on the device with the same float ops.
void mcu_row_coeffs(const uint8_t* rgba, int W, int H, int my, const float qy[64], const float qc[64],
                    int16_t* out) {
    const int mcux = (W + 15) / 16;
    float Y[4][64], Cb[64], Cr[64];
    for (int mx = 0; mx < mcux; ++mx) {
        float cbs[16][16], crs[16][16];
        for (int yy = 0; yy < 16; ++yy) {
            const int sy = std::min(my * 16 + yy, H - 1);
            for (int xx = 0; xx < 16; ++xx) {
                const int sx = std::min(mx * 16 + xx, W - 1);
                const uint8_t* p = rgba + 4 * ((size_t)sy * W + sx);
                const float r = p[0], g = p[1], b = p[2];
                const float y = 0.299f * r + 0.587f * g + 0.114f * b;
                Y[(yy >> 3) * 2 + (xx >> 3)][8 * (yy & 7) + (xx & 7)] = y - 128.0f;
                cbs[yy][xx] = -0.168735892f * r - 0.331264108f * g + 0.5f * b;
                crs[yy][xx] = 0.5f * r - 0.418687589f * g - 0.081312411f * b;
            }
        }
        for (int yy = 0; yy < 8; ++yy)
            for (int xx = 0; xx < 8; ++xx) {
                Cb[8 * yy + xx] = 0.25f * (cbs[2 * yy][2 * xx] + cbs[2 * yy][2 * xx + 1] + cbs[2 * yy + 1][2 * xx] +
                                           cbs[2 * yy + 1][2 * xx + 1]);
                Cr[8 * yy + xx] = 0.25f * (crs[2 * yy][2 * xx] + crs[2 * yy][2 * xx + 1] + crs[2 * yy + 1][2 * xx] +
                                           crs[2 * yy + 1][2 * xx + 1]);
            }
        int16_t* o = out + (size_t)mx * 6 * 64;
        for (int k = 0; k < 4; ++k) fdct_quant(Y[k], qy, o + 64 * k);
        fdct_quant(Cb, qc, o + 64 * 4);
        fdct_quant(Cr, qc, o + 64 * 5);
    }
}

// The same for a grey file's MCU row `my` (8 pixel rows): coefficients
// [mcux][64], one block an MCU, Y the grey code (grey.h) of the pixel.
void mcu_row_coeffs_grey(const uint8_t* rgba, int W, int H, int my, const float qy[64], int16_t* out) {
    const int mcux = (W + 7) / 8;
    float Y[64];
    for (int mx = 0; mx < mcux; ++mx) {
        for (int yy = 0; yy < 8; ++yy) {
            const int sy = std::min(my * 8 + yy, H - 1);
            for (int xx = 0; xx < 8; ++xx) {
                const int sx = std::min(mx * 8 + xx, W - 1);
                const uint8_t* p = rgba + 4 * ((size_t)sy * W + sx);
                Y[8 * yy + xx] = (float)grey8(p[0], p[1], p[2]) - 128.0f;
            }
        }
        fdct_quant(Y, qy, out + (size_t)mx * 64);
    }
}

// Huffman-code one MCU row (one restart interval) from its coefficients.
void entropy_mcu_row(const int16_t* coeffs, int mcux, std::vector<uint8_t>& out, bool grey = false) {
    const Tables& T = tables();
    BitWriter bw(out);
    int pred[3] = {0, 0, 0};
    if (grey) {
        for (int mx = 0; mx < mcux; ++mx) encode_block(bw, coeffs + (size_t)mx * 64, pred[0], T.dc[0], T.ac[0]);
        bw.flush();
        return;
    }
    for (int mx = 0; mx < mcux; ++mx) {
        const int16_t* o = coeffs + (size_t)mx * 6 * 64;
        for (int k = 0; k < 4; ++k) encode_block(bw, o + 64 * k, pred[0], T.dc[0], T.ac[0]);
        encode_block(bw, o + 64 * 4, pred[1], T.dc[1], T.ac[1]);
        encode_block(bw, o + 64 * 5, pred[2], T.dc[1], T.ac[1]);
    }
    bw.flush();
}

// grey: one component 1x1 with the luma tables, MCUs of 8x8 pixels.
void jpeg_header(int W, int H, const uint8_t* ql, const uint8_t* qc, std::vector<uint8_t>& out, bool grey = false) {
    // SOI + APP0 JFIF
    const uint8_t soi_app0[] = {0xFF, 0xD8, 0xFF, 0xE0, 0x00, 0x10, 'J', 'F', 'I', 'F', 0x00,
                                0x01, 0x01, 0x00, 0x00, 0x01, 0x00, 0x01, 0x00, 0x00};
    out.insert(out.end(), soi_app0, soi_app0 + sizeof soi_app0);
    // DQT (tables in zigzag order)
    for (int t = 0; t < (grey ? 1 : 2); ++t) {
        const uint8_t* q = t ? qc : ql;
        out.push_back(0xFF); out.push_back(0xDB);
        put16(out, 67);
        out.push_back((uint8_t)t);
        for (int k = 0; k < 64; ++k) out.push_back(q[kZigzag[k]]);
    }
    if (grey) {
        out.push_back(0xFF); out.push_back(0xC0);
        put16(out, 11);
        out.push_back(8);
        put16(out, H);
        put16(out, W);
        const uint8_t comp[4] = {1, 1, 0x11, 0};
        out.insert(out.end(), comp, comp + 4);
        write_dht(out, 0, 0, kDcLumBits, kDcLumVal);
        write_dht(out, 1, 0, kAcLumBits, kAcLumVal);
        out.push_back(0xFF); out.push_back(0xDD);
        put16(out, 4);
        put16(out, (W + 7) / 8);
        const uint8_t sos[] = {0xFF, 0xDA, 0x00, 0x08, 0x01, 1, 0x00, 0x00, 0x3F, 0x00};
        out.insert(out.end(), sos, sos + sizeof sos);
        return;
    }
    // SOF0: 3 components, Y 2x2, Cb/Cr 1x1
    out.push_back(0xFF); out.push_back(0xC0);
    put16(out, 17);
    out.push_back(8);
    put16(out, H);
    put16(out, W);
    out.push_back(3);
    const uint8_t comps[9] = {1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1};
    out.insert(out.end(), comps, comps + 9);
    write_dht(out, 0, 0, kDcLumBits, kDcLumVal);
    write_dht(out, 1, 0, kAcLumBits, kAcLumVal);
    write_dht(out, 0, 1, kDcChrBits, kDcChrVal);
    write_dht(out, 1, 1, kAcChrBits, kAcChrVal);
    // DRI: one restart interval per MCU row
    out.push_back(0xFF); out.push_back(0xDD);
    put16(out, 4);
    put16(out, (W + 15) / 16);
    // SOS
    const uint8_t sos[] = {0xFF, 0xDA, 0x00, 0x0C, 0x03, 1, 0x00, 2, 0x11, 3, 0x11, 0x00, 0x3F, 0x00};
    out.insert(out.end(), sos, sos + sizeof sos);
}

// Run fn(my) for every MCU row on `threads` host threads.
template <typename Fn>
void for_rows(int mcuy, int threads, Fn fn) {
    if (threads <= 0) threads = encoder_threads();
    threads = std::max(1, std::min(threads, mcuy));
    if (threads == 1) {
        for (int my = 0; my < mcuy; ++my) fn(my);
        return;
    }
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; ++t)
        pool.emplace_back([&, t] {
            for (int my = t; my < mcuy; my += threads) fn(my);
        });
    for (auto& th : pool) th.join();
}

void join_rows(std::vector<std::vector<uint8_t>>& rows, std::vector<uint8_t>& out) {
    const int mcuy = (int)rows.size();
    for (int my = 0; my < mcuy; ++my) {
        out.insert(out.end(), rows[my].begin(), rows[my].end());
        if (my + 1 < mcuy) {
            out.push_back(0xFF);
            out.push_back((uint8_t)(0xD0 + (my & 7)));
        }
    }
    out.push_back(0xFF); out.push_back(0xD9);
}

// --------------------------------------------------------------- PNG ------
void png_chunk(std::vector<uint8_t>& o, const char* type, const uint8_t* data, size_t n) {
    const uint32_t len = (uint32_t)n;
    o.push_back((uint8_t)(len >> 24)); o.push_back((uint8_t)(len >> 16));
    o.push_back((uint8_t)(len >> 8)); o.push_back((uint8_t)len);
    const size_t start = o.size();
    o.insert(o.end(), type, type + 4);
    if (n) o.insert(o.end(), data, data + n);
    const uint32_t crc = (uint32_t)crc32(0L, o.data() + start, (uInt)(o.size() - start));
    o.push_back((uint8_t)(crc >> 24)); o.push_back((uint8_t)(crc >> 16));
    o.push_back((uint8_t)(crc >> 8)); o.push_back((uint8_t)crc);
}

}  // namespace

void jpeg_tables(int quality, JpegTables& t) {
    quant_table(kStdLuma, quality, t.ql);
    quant_table(kStdChroma, quality, t.qc);
    for (int i = 0; i < 64; ++i) {  // quantisation folded as a multiply by 1/q
        t.dct[i] = dct().c[i / 8][i % 8];
        t.qinv_l[i] = 1.0f / (float)t.ql[i];
        t.qinv_c[i] = 1.0f / (float)t.qc[i];
    }
}

void jpeg_header_bytes(int W, int H, int quality, std::vector<uint8_t>& out, bool grey) {
    JpegTables t;
    jpeg_tables(quality, t);
    out.clear();
    jpeg_header(W, H, t.ql, t.qc, out, grey);
}

void jpeg_huff_tables(uint32_t out[4 * 256]) {
    const Tables& T = tables();
    const HuffTable* order[4] = {&T.dc[0], &T.ac[0], &T.dc[1], &T.ac[1]};
    for (int t = 0; t < 4; ++t)
        for (int s = 0; s < 256; ++s) out[256 * t + s] = (uint32_t)order[t]->code[s] | ((uint32_t)order[t]->len[s] << 16);
}

size_t jpeg_coeff_count(int W, int H, bool grey) {
    return grey ? (size_t)((W + 7) / 8) * ((H + 7) / 8) * 64 : (size_t)((W + 15) / 16) * ((H + 15) / 16) * 6 * 64;
}

bool encode_jpeg(const uint8_t* rgba, int W, int H, int quality, std::vector<uint8_t>& out, int threads, bool grey) {
    if (W <= 0 || H <= 0 || W > 65535 || H > 65535) return false;
    JpegTables t;
    jpeg_tables(quality, t);
    if (grey) {
        const int mcux = (W + 7) / 8, mcuy = (H + 7) / 8;
        out.clear();
        out.reserve((size_t)W * H / 4);
        jpeg_header(W, H, t.ql, t.qc, out, true);
        std::vector<std::vector<uint8_t>> rows((size_t)mcuy);
        for_rows(mcuy, threads, [&](int my) {
            std::vector<int16_t> c((size_t)mcux * 64);
            mcu_row_coeffs_grey(rgba, W, H, my, t.qinv_l, c.data());
            rows[my].reserve((size_t)mcux * 48);
            entropy_mcu_row(c.data(), mcux, rows[my], true);
        });
        join_rows(rows, out);
        return true;
    }
    const int mcux = (W + 15) / 16, mcuy = (H + 15) / 16;
    out.clear();
    out.reserve((size_t)W * H / 2);
    jpeg_header(W, H, t.ql, t.qc, out);
    std::vector<std::vector<uint8_t>> rows((size_t)mcuy);
    for_rows(mcuy, threads, [&](int my) {
        std::vector<int16_t> c((size_t)mcux * 6 * 64);
        mcu_row_coeffs(rgba, W, H, my, t.qinv_l, t.qinv_c, c.data());
        rows[my].reserve((size_t)mcux * 256);
        entropy_mcu_row(c.data(), mcux, rows[my]);
    });
    join_rows(rows, out);
    return true;
}

bool encode_jpeg_coeffs(const int16_t* coeffs, int W, int H, int quality, std::vector<uint8_t>& out,
                        int threads) {
    if (W <= 0 || H <= 0 || W > 65535 || H > 65535) return false;
    JpegTables t;
    jpeg_tables(quality, t);
    const int mcux = (W + 15) / 16, mcuy = (H + 15) / 16;
    out.clear();
    out.reserve((size_t)W * H / 2);
    jpeg_header(W, H, t.ql, t.qc, out);
    std::vector<std::vector<uint8_t>> rows((size_t)mcuy);
    for_rows(mcuy, threads, [&](int my) {
        rows[my].reserve((size_t)mcux * 256);
        entropy_mcu_row(coeffs + (size_t)my * mcux * 6 * 64, mcux, rows[my]);
    });
    join_rows(rows, out);
    return true;
}

int png_zlib_level(int compression) {
    const int level = (int)((float)compression / 11.1111f);
    return std::min(std::max(level, 0), 9);
}

// PNG (8-bit RGBA, filter Sub on every row). The zlib stream is deflated in
// bands of rows on host threads, pigz-style: each band is a raw deflate stream
// ended with a sync flush (an empty stored block, byte-aligned), the last one
// with the final block; concatenated they form one deflate stream, wrapped in
// the zlib header and the Adler-32 of the whole image (adler32_combine of the
// bands'). A band restarts the 32 KB match window, which costs a little ratio
// and no correctness. A 1080p 02 frame: one thread took most of the frame's
// time on the host, more than the GPU's.
// channels: 4 RGBA (colour type 6), 3 RGB (2), 1 grey (0, the grey code of grey.h).
// adaptive (rr_set_png_compression 0 .. 100): libpng's adaptive filter on every
// row (png_filter.h) and the zlib header's level hint as zlib writes it; a row
// is filtered against the image's row above, also across the thread bands.
bool encode_png(const uint8_t* rgba, int W, int H, std::vector<uint8_t>& out, int level, int threads, int channels,
                bool adaptive) {
    if (W <= 0 || H <= 0 || (channels != 1 && channels != 3 && channels != 4)) return false;
    if (level < 0 || level > 9) return false;
    std::vector<uint8_t> packed;  // the image with the file's channels
    if (channels != 4) {
        packed.resize((size_t)W * H * channels);
        for (size_t i = 0, n = (size_t)W * H; i < n; ++i) {
            const uint8_t* p = rgba + 4 * i;
            if (channels == 1) packed[i] = (uint8_t)grey8(p[0], p[1], p[2]);
            else std::memcpy(&packed[3 * i], p, 3);
        }
        rgba = packed.data();
    }
    const size_t C = (size_t)channels;
    const size_t stride = (size_t)W * C;
    std::vector<uint8_t> raw((stride + 1) * H);
    if (threads <= 0) threads = encoder_threads();
    const int bands = std::max(1, std::min(threads, H / 16));  // >= 16 rows a band
    std::vector<std::vector<uint8_t>> zb(bands);
    std::vector<uLong> adl(bands), len(bands);
    std::vector<int> ok(bands, 0);
    auto band = [&](int b) {
        const int y0 = (int)((long)H * b / bands), y1 = (int)((long)H * (b + 1) / bands);
        for (int y = y0; y < y1; ++y) {
            uint8_t* dst = &raw[(stride + 1) * y];
            const uint8_t* src = rgba + stride * y;
            if (adaptive) {
                const uint8_t* up = y > 0 ? src - stride : nullptr;
                const uint32_t type = png_pick_row(src, up, stride, C, (size_t)H);
                dst[0] = (uint8_t)type;
                png_filter_row(type, src, up, stride, C, dst + 1);
                continue;
            }
            dst[0] = 1;
            for (size_t x = 0; x < stride; ++x) dst[1 + x] = (uint8_t)(src[x] - (x >= C ? src[x - C] : 0));
        }
        const uint8_t* in = &raw[(stride + 1) * y0];
        const uLong n = (uLong)((stride + 1) * (size_t)(y1 - y0));
        z_stream zs{};
        if (deflateInit2(&zs, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return;
        zb[b].resize(deflateBound(&zs, n) + 16);
        zs.next_in = const_cast<Bytef*>(in);
        zs.avail_in = (uInt)n;
        zs.next_out = zb[b].data();
        zs.avail_out = (uInt)zb[b].size();
        const int rc = deflate(&zs, b == bands - 1 ? Z_FINISH : Z_SYNC_FLUSH);
        const bool done = b == bands - 1 ? rc == Z_STREAM_END : (rc == Z_OK && zs.avail_in == 0);
        zb[b].resize(zb[b].size() - zs.avail_out);
        deflateEnd(&zs);
        adl[b] = adler32(adler32(0L, Z_NULL, 0), in, (uInt)n);
        len[b] = n;
        ok[b] = done ? 1 : 0;
    };
    if (bands == 1) {
        band(0);
    } else {
        std::vector<std::thread> pool;
        for (int b = 0; b < bands; ++b) pool.emplace_back(band, b);
        for (auto& t : pool) t.join();
    }
    // zlib header: deflate, 32 KB window, no dictionary; FLEVEL says 0 ("fastest") unless the setting chose the level
    const uint8_t flg = !adaptive || level < 2 ? 0x01 : level < 6 ? 0x5E : level == 6 ? 0x9C : 0xDA;
    std::vector<uint8_t> z = {0x78, flg};
    uLong a = adler32(0L, Z_NULL, 0);
    for (int b = 0; b < bands; ++b) {
        if (!ok[b]) return false;
        z.insert(z.end(), zb[b].begin(), zb[b].end());
        a = adler32_combine(a, adl[b], (z_off_t)len[b]);
    }
    for (int k = 3; k >= 0; --k) z.push_back((uint8_t)(a >> (8 * k)));
    out.clear();
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
    out.insert(out.end(), sig, sig + 8);
    uint8_t ihdr[13] = {(uint8_t)(W >> 24), (uint8_t)(W >> 16), (uint8_t)(W >> 8), (uint8_t)W,
                        (uint8_t)(H >> 24), (uint8_t)(H >> 16), (uint8_t)(H >> 8), (uint8_t)H,
                        8, (uint8_t)(channels == 4 ? 6 : channels == 3 ? 2 : 0), 0, 0, 0};
    png_chunk(out, "IHDR", ihdr, 13);
    png_chunk(out, "IDAT", z.data(), z.size());
    png_chunk(out, "IEND", nullptr, 0);
    return true;
}

void png_wrap_stream(int W, int H, const uint8_t* zs, size_t n, const uint32_t* band_tab, int nbands,
                     std::vector<uint8_t>& out, int depth, int color_type) {
    uLong a = adler32(0L, Z_NULL, 0);
    for (int b = 0; b < nbands; ++b) a = adler32_combine(a, band_tab[2 * b], (z_off_t)band_tab[2 * b + 1]);
    std::vector<uint8_t> z(zs, zs + n);
    for (int k = 3; k >= 0; --k) z.push_back((uint8_t)(a >> (8 * k)));
    out.clear();
    out.reserve(z.size() + 64);
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
    out.insert(out.end(), sig, sig + 8);
    uint8_t ihdr[13] = {(uint8_t)(W >> 24), (uint8_t)(W >> 16), (uint8_t)(W >> 8), (uint8_t)W,
                        (uint8_t)(H >> 24), (uint8_t)(H >> 16), (uint8_t)(H >> 8), (uint8_t)H,
                        (uint8_t)depth, (uint8_t)color_type, 0, 0, 0};
    png_chunk(out, "IHDR", ihdr, 13);
    png_chunk(out, "IDAT", z.data(), z.size());
    png_chunk(out, "IEND", nullptr, 0);
}

// --------------------------------------------------------------- EXR ------
namespace {
void put_le(std::vector<uint8_t>& o, uint64_t v, int bytes) {
    for (int k = 0; k < bytes; ++k) o.push_back((uint8_t)(v >> (8 * k)));
}
void put_str(std::vector<uint8_t>& o, const char* s) {
    for (; *s; ++s) o.push_back((uint8_t)*s);
    o.push_back(0);
}
void exr_attr(std::vector<uint8_t>& o, const char* name, const char* type, const std::vector<uint8_t>& value) {
    put_str(o, name);
    put_str(o, type);
    put_le(o, value.size(), 4);
    o.insert(o.end(), value.begin(), value.end());
}
}  // namespace

namespace {
// The file's magic, version and header with the compression attribute `compression`.
bool exr_header_bytes(int W, int H, int pixel_type, int channels, int compression, std::vector<uint8_t>& out) {
    if (channels != 1 && channels != 3 && channels != 4) return false;
    out.clear();
    const uint8_t start[8] = {0x76, 0x2F, 0x31, 0x01, 2, 0, 0, 0};
    out.insert(out.end(), start, start + 8);
    std::vector<uint8_t> v;
    const char* const names[4] = {"A", "B", "G", "R"};
    for (int k = 4 - channels; k < 4; ++k) {
        put_str(v, channels == 1 ? "Y" : names[k]);
        put_le(v, (uint32_t)pixel_type, 4);  // 1 HALF, 2 FLOAT
        put_le(v, 0, 4);                     // pLinear, 3 reserved bytes
        put_le(v, 1, 4);  // xSampling
        put_le(v, 1, 4);  // ySampling
    }
    v.push_back(0);
    exr_attr(out, "channels", "chlist", v);
    exr_attr(out, "compression", "compression", {(uint8_t)compression});  // 3: ZIP, 16 scanlines
    v.clear();
    put_le(v, 0, 4);
    put_le(v, 0, 4);
    put_le(v, (uint32_t)(W - 1), 4);
    put_le(v, (uint32_t)(H - 1), 4);
    exr_attr(out, "dataWindow", "box2i", v);
    exr_attr(out, "displayWindow", "box2i", v);
    exr_attr(out, "lineOrder", "lineOrder", {0});
    const std::vector<uint8_t> one = {0, 0, 0x80, 0x3F};  // 1.0f
    exr_attr(out, "pixelAspectRatio", "float", one);
    exr_attr(out, "screenWindowCenter", "v2f", std::vector<uint8_t>(8, 0));
    exr_attr(out, "screenWindowWidth", "float", one);
    out.push_back(0);
    return true;
}
}  // namespace

bool exr_wrap_stream(int W, int H, const uint8_t* data, size_t n, const uint32_t* chunk_tab, int nchunks,
                     std::vector<uint8_t>& out, int pixel_type, int channels, int compression) {
    const uint32_t row_bytes = (pixel_type == 2 ? 4u : 2u) * (uint32_t)channels * (uint32_t)W;  // planes of FLOAT or HALF
    // the bytes of a scanline as the chunk's stream holds them: PXR24 (5) 3 of a float's 4
    const uint32_t front_row_bytes = compression == 5 && pixel_type == 2 ? row_bytes / 4u * 3u : row_bytes;
    std::vector<uint8_t> head;
    if (!exr_header_bytes(W, H, pixel_type, channels, compression, head)) return false;
    out.clear();
    out.reserve(n + 512 + (size_t)nchunks * 22);
    out = head;
    uint64_t at = out.size() + 8ull * (uint64_t)nchunks;
    for (int b = 0; b < nchunks; ++b) {
        put_le(out, at, 8);
        at += 8 + chunk_tab[4 * b + 1] + (chunk_tab[4 * b] == 0 ? 6 : 0);
    }
    size_t src = 0;
    for (int b = 0; b < nchunks; ++b) {
        const uint32_t mode = chunk_tab[4 * b], len = chunk_tab[4 * b + 1], adler = chunk_tab[4 * b + 2];
        if (src + len > n) return false;
        // a raw chunk is its scanlines' bytes, a coded one is smaller
        const uint32_t rows = (uint32_t)std::min(16, H - b * 16);
        const uint32_t raw = row_bytes * rows;
        if (chunk_tab[4 * b + 3] != front_row_bytes * rows || (mode == 0 ? len + 6 >= raw : len != raw)) return false;
        put_le(out, (uint32_t)(b * 16), 4);
        put_le(out, mode == 0 ? len + 6 : len, 4);
        if (mode == 0) {
            out.push_back(0x78);
            out.push_back(0x01);
        }
        out.insert(out.end(), data + src, data + src + len);
        if (mode == 0)
            for (int k = 3; k >= 0; --k) out.push_back((uint8_t)(adler >> (8 * k)));
        src += len;
    }
    return src == n;
}

bool exr_wrap_rows(int W, int H, const uint8_t* data, size_t n, const uint32_t* row_tab, std::vector<uint8_t>& out,
                   int pixel_type, int channels, int compression) {
    const uint32_t row_bytes = (pixel_type == 2 ? 4u : 2u) * (uint32_t)channels * (uint32_t)W;
    if (!exr_header_bytes(W, H, pixel_type, channels, compression, out)) return false;
    out.reserve(out.size() + n + (size_t)H * 16);
    uint64_t at = out.size() + 8ull * (uint64_t)H;
    for (int y = 0; y < H; ++y) {
        put_le(out, at, 8);
        at += 8 + (row_tab ? row_tab[2 * y + 1] : row_bytes);
    }
    size_t src = 0;
    for (int y = 0; y < H; ++y) {
        const uint32_t mode = row_tab ? row_tab[2 * y] : 1u, len = row_tab ? row_tab[2 * y + 1] : row_bytes;
        // a raw chunk is its scanline's bytes, a coded one is smaller and not empty
        if (src + len > n || (mode == 0 ? len >= row_bytes || len == 0 : len != row_bytes)) return false;
        put_le(out, (uint32_t)y, 4);
        put_le(out, len, 4);
        out.insert(out.end(), data + src, data + src + len);
        src += len;
    }
    return src == n;
}

// ------------------------------------------------- run-length packets ------
namespace {

// The packets of one row of W elements, T::kElemBytes bytes each, by the rule
// of rle_rule.h with T's numbers, appended to out. Stated as a walk over the
// maximal runs; the device packer (rle_device.hpp) states it as window
// functions on eq bits and writes the same bytes.
template <class T>
void rle_pack_row(const uint8_t* row, size_t W, std::vector<uint8_t>& out) {
    constexpr size_t c = T::kElemBytes;
    // a stretch of n elements from element `from`: packets of the kind's cap, then the remainder
    auto put_stretch = [&](size_t from, size_t n, bool run) {
        const size_t cap = rle_packet_cap<T>(run);
        for (size_t at = 0; at < n; at += cap) {
            const size_t count = std::min(cap, n - at);
            out.push_back((uint8_t)T::header(run, (uint32_t)count));
            const uint8_t* el = row + c * (from + at);
            out.insert(out.end(), el, el + c * (run ? 1 : count));
        }
    };
    size_t lit = 0;  // first element of the open literal stretch
    for (size_t x = 0; x < W;) {
        size_t e = x + 1;  // the maximal run [x, e)
        while (e < W && std::memcmp(row + c * e, row + c * x, c) == 0) ++e;
        if (e - x >= T::kMinRun) {
            put_stretch(lit, x - lit, false);
            put_stretch(x, e - x, true);
            lit = e;
        }
        x = e;
    }
    put_stretch(lit, W - lit, false);
}

}  // namespace

void exr_rle_pack(const uint8_t* bytes, size_t n, std::vector<uint8_t>& out) { rle_pack_row<ExrRle>(bytes, n, out); }

// ------------------------------------------------------------- TARGA ------
void tga_header_bytes(int W, int H, int C, bool rle, std::vector<uint8_t>& out) {
    out.clear();
    out.push_back(0);                                          // no image id
    out.push_back(0);                                          // no colour map
    out.push_back((uint8_t)((C == 1 ? 3 : 2) + (rle ? 8 : 0)));  // 2 true colour, 3 grey, + 8 run-length coded
    for (int k = 0; k < 5; ++k) out.push_back(0);              // colour map specification
    put_le(out, 0, 2);                                         // x origin
    put_le(out, 0, 2);                                         // y origin
    put_le(out, (uint32_t)W, 2);
    put_le(out, (uint32_t)H, 2);
    out.push_back((uint8_t)(8 * C));                           // bits a pixel
    out.push_back(C == 4 ? 8 : 0);                             // alpha bits; bit 5 clear: bottom-left origin
}

bool encode_tga(const uint8_t* rgba, int W, int H, int C, bool rle, std::vector<uint8_t>& out) {
    const uint64_t bound = tga_body_max_bytes(W, H, C, rle);
    if (!rgba || bound == 0) return false;
    tga_header_bytes(W, H, C, rle, out);
    out.reserve(out.size() + (size_t)bound);
    std::vector<uint8_t> row((size_t)W * C);
    const size_t c = (size_t)C;
    for (int y = H - 1; y >= 0; --y) {  // bottom row first
        const uint8_t* src = rgba + (size_t)y * W * 4;
        for (int x = 0; x < W; ++x) {
            const uint8_t* p = src + 4 * (size_t)x;
            uint8_t* q = row.data() + c * x;
            if (C == 1) {
                q[0] = (uint8_t)grey8(p[0], p[1], p[2]);
            } else {
                q[0] = p[2], q[1] = p[1], q[2] = p[0];
                if (C == 4) q[3] = p[3];
            }
        }
        if (!rle) {
            out.insert(out.end(), row.begin(), row.end());
            continue;
        }
        if (C == 1) rle_pack_row<TgaRle<1>>(row.data(), (size_t)W, out);
        else if (C == 3) rle_pack_row<TgaRle<3>>(row.data(), (size_t)W, out);
        else rle_pack_row<TgaRle<4>>(row.data(), (size_t)W, out);
    }
    return out.size() - kTgaHeaderBytes <= bound;
}

// --------------------------------------------------------------- HDR ------
void hdr_header_bytes(int W, int H, std::vector<uint8_t>& out) {
    const std::string text =
        "#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y " + std::to_string(H) + " +X " + std::to_string(W) + "\n";
    out.assign(text.begin(), text.end());
}

bool encode_hdr(const float* rgba, int W, int H, int C, std::vector<uint8_t>& out) {
    const uint64_t bound = hdr_body_max_bytes(W, H);
    if (!rgba || bound == 0 || (C != 1 && C != 3)) return false;
    hdr_header_bytes(W, H, out);
    const size_t head = out.size();
    out.reserve(head + (size_t)bound);
    auto bits = [](float v) {
        uint32_t u;
        std::memcpy(&u, &v, sizeof u);
        return u;
    };
    std::vector<uint8_t> quads((size_t)W * 4), plane((size_t)W);
    for (int y = 0; y < H; ++y) {  // top row first
        const float* src = rgba + (size_t)y * W * 4;
        for (int x = 0; x < W; ++x) {
            const float* p = src + 4 * (size_t)x;
            uint32_t q;
            if (C == 1) {
                const uint32_t l = bits(luma709(p[0], p[1], p[2]));
                q = hdr_quad(l, l, l);
            } else {
                q = hdr_quad(bits(p[0]), bits(p[1]), bits(p[2]));
            }
            for (int k = 0; k < 4; ++k) quads[4 * (size_t)x + k] = (uint8_t)(q >> (8 * k));
        }
        if (hdr_row_flat(W)) {
            out.insert(out.end(), quads.begin(), quads.end());
            continue;
        }
        const uint8_t marker[4] = {2, 2, (uint8_t)(W >> 8), (uint8_t)W};
        out.insert(out.end(), marker, marker + 4);
        for (int k = 0; k < 4; ++k) {
            for (int x = 0; x < W; ++x) plane[(size_t)x] = quads[4 * (size_t)x + k];
            rle_pack_row<HdrRle>(plane.data(), (size_t)W, out);
        }
    }
    return out.size() - head <= bound;
}

// -------------------------------------------------------------- IRIS ------
void iris_header_bytes(int W, int H, int C, std::vector<uint8_t>& out) {
    out.assign(kIrisHeaderBytes, 0);  // name, colour map id 0 and the rest of the header stay 0
    auto put_be16 = [&](size_t at, uint32_t v) { out[at] = (uint8_t)(v >> 8), out[at + 1] = (uint8_t)v; };
    put_be16(0, 474);                // the magic number
    out[2] = 1;                      // run-length coded
    out[3] = 1;                      // a byte a channel
    put_be16(4, C == 1 ? 2 : 3);     // dimension
    put_be16(6, (uint32_t)W);
    put_be16(8, (uint32_t)H);
    put_be16(10, (uint32_t)C);
    out[19] = 255;                   // pixmin 0 at 12, pixmax 255 at 16
}

bool encode_iris(const uint8_t* rgba, int W, int H, int C, std::vector<uint8_t>& out) {
    const uint64_t bound = iris_body_max_bytes(W, H, C);
    if (!rgba || bound == 0) return false;
    iris_header_bytes(W, H, C, out);
    const size_t n = (size_t)H * (size_t)C;
    out.reserve(out.size() + (size_t)bound);
    out.resize(out.size() + (size_t)iris_table_bytes((uint64_t)H, (uint64_t)C), 0);
    auto put_be32 = [&](size_t at, uint64_t v) {
        for (int k = 0; k < 4; ++k) out[at + (size_t)k] = (uint8_t)(v >> (8 * (3 - k)));
    };
    std::vector<uint8_t> plane((size_t)W);
    for (int f = 0; f < H; ++f) {  // file row f: bottom row first
        const uint8_t* src = rgba + (size_t)(H - 1 - f) * W * 4;
        for (int z = 0; z < C; ++z) {
            for (int x = 0; x < W; ++x) {
                const uint8_t* p = src + 4 * (size_t)x;
                plane[(size_t)x] = C == 1 ? (uint8_t)grey8(p[0], p[1], p[2]) : p[z];
            }
            const size_t start = out.size();
            rle_pack_row<IrisRle>(plane.data(), (size_t)W, out);
            out.push_back(0);  // the terminator
            const size_t entry = (size_t)f + (size_t)z * (size_t)H;
            put_be32(kIrisHeaderBytes + 4 * entry, start);
            put_be32(kIrisHeaderBytes + 4 * (n + entry), out.size() - start);
        }
    }
    return out.size() - kIrisHeaderBytes <= bound;
}

// -------------------------------------------------------------- WEBP ------
namespace {

// An LSB-first bit stream appended to a byte vector.
struct WebpBits {
    std::vector<uint8_t>& out;
    uint64_t acc = 0;
    int n = 0;
    void put(uint32_t v, int nb) {  // the low nb <= 32 bits of v
        acc |= (uint64_t)v << n;
        n += nb;
        for (; n >= 8; n -= 8, acc >>= 8) out.push_back((uint8_t)acc);
    }
    void flush() {
        if (n > 0) out.push_back((uint8_t)acc);
        acc = 0, n = 0;
    }
    // A simple code of k = 1 or 2 symbols, s0 < s1 < 256.
    void simple(int k, uint32_t s0, uint32_t s1) {
        put(1u, 1);
        put((uint32_t)(k - 1), 1);
        put(s0 > 1u ? 1u : 0u, 1);
        put(s0, s0 > 1u ? 8 : 1);
        if (k == 2) put(s1, 8);
    }
};

// Code lengths (<= maxbits) of an alphabet with at least two nonzero counts:
// deflate.hip's build_lengths, step for step. Symbols ranked by (count, index),
// the tree by the two-queue merge, depths capped, the Kraft sum repaired by
// moving leaves down, lengths handed out by rank.
void webp_lengths(const uint32_t* freq, int n, int maxbits, uint8_t* lens) {
    std::vector<int> order;
    for (int s = 0; s < n; ++s) {
        lens[s] = 0;
        if (freq[s]) order.push_back(s);
    }
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return freq[a] < freq[b]; });
    const int nu = (int)order.size();
    std::vector<uint32_t> iw((size_t)nu);
    std::vector<int> lpar((size_t)nu), ipar((size_t)nu), idepth((size_t)nu);
    int li = 0, ii = 0, ni = 0;
    for (int k = 0; k + 1 < nu; ++k) {
        uint32_t w = 0;
        for (int pick = 0; pick < 2; ++pick) {
            if (li < nu && (ii >= ni || freq[order[(size_t)li]] <= iw[(size_t)ii])) {
                w += freq[order[(size_t)li]];
                lpar[(size_t)li++] = ni;
            } else {
                w += iw[(size_t)ii];
                ipar[(size_t)ii++] = ni;
            }
        }
        iw[(size_t)ni++] = w;
    }
    int count[33] = {};
    if (ni > 0) idepth[(size_t)ni - 1] = 0;
    for (int k = ni - 2; k >= 0; --k) idepth[(size_t)k] = idepth[(size_t)ipar[(size_t)k]] + 1;
    for (int i = 0; i < nu; ++i) count[std::min(idepth[(size_t)lpar[(size_t)i]] + 1, maxbits)] += 1;
    uint32_t total = 0;
    for (int i = maxbits; i >= 1; --i) total += (uint32_t)count[i] << (maxbits - i);
    while (total > (1u << maxbits)) {
        count[maxbits] -= 1;
        for (int i = maxbits - 1; i >= 1; --i)
            if (count[i]) {
                count[i] -= 1;
                count[i + 1] += 2;
                break;
            }
        total -= 1;
    }
    int j = nu;
    for (int i = 1; i <= maxbits; ++i)
        for (int l = count[i]; l > 0; --l) lens[order[(size_t)--j]] = (uint8_t)i;
}

// Canonical codes of lens[0 .. n), bit-reversed for the LSB-first stream:
// code | length << 16, as deflate.hip's assign_codes.
void webp_assign_codes(const uint8_t* lens, int n, uint32_t* codes) {
    uint32_t next[17];
    int count[17] = {};
    for (int s = 0; s < n; ++s) count[lens[s]] += 1;
    count[0] = 0;
    uint32_t code = 0;
    next[0] = 0;
    for (int i = 1; i <= 16; ++i) {
        code = (code + (uint32_t)count[i - 1]) << 1;
        next[i] = code;
    }
    for (int s = 0; s < n; ++s) {
        const int l = lens[s];
        uint32_t c = l ? next[l]++ : 0u, r = 0;
        for (int k = 0; k < l; ++k) r |= ((c >> k) & 1u) << (l - 1 - k);
        codes[s] = l ? (r | (uint32_t)l << 16) : 0u;
    }
}

// One alphabet's code into the header and the table (code | length << 16).
void webp_write_code(WebpBits& b, const uint32_t* freq, int n, uint32_t* codes) {
    uint32_t nu = 0, lo = 0, hi = 0;
    for (int s = 0; s < n; ++s)
        if (freq[s]) {
            if (!nu++) lo = (uint32_t)s;
            hi = (uint32_t)s;
        }
    for (int s = 0; s < n; ++s) codes[s] = 0u;
    if (nu == 0u || (nu <= 2u && hi < 256u)) {
        b.simple(nu == 2u ? 2 : 1, lo, hi);
        if (nu == 2u) codes[lo] = 0u | 1u << 16, codes[hi] = 1u | 1u << 16;
        return;
    }
    std::vector<uint8_t> lens((size_t)n);
    webp_lengths(freq, n, kWebpMaxBits, lens.data());
    uint32_t clfreq[19] = {}, clcode[19] = {};
    uint8_t cllen[19] = {};
    for (int s = 0; s < n; ++s) clfreq[lens[(size_t)s]] += 1u;
    int cu = 0;
    for (int k = 0; k < 19; ++k)
        if (clfreq[k]) ++cu, cllen[k] = 1;  // its only used symbol: length 1, and its uses take no bits
    if (cu >= 2) {
        webp_lengths(clfreq, 19, kWebpClMaxBits, cllen);
        webp_assign_codes(cllen, 19, clcode);
    }
    webp_assign_codes(lens.data(), n, codes);
    b.put(0u, 1);
    b.put(19u - 4u, 4);
    for (int k = 0; k < 19; ++k) b.put(cllen[webp_cl_order(k)], 3);
    b.put(0u, 1);  // every symbol's length follows
    for (int s = 0; s < n; ++s) {
        const uint32_t c = clcode[lens[(size_t)s]];
        b.put(c & 0xFFFFu, (int)(c >> 16));
    }
}

}  // namespace

void webp_wrap_stream(const uint8_t* payload, size_t len, std::vector<uint8_t>& out) {
    const size_t pad = len & 1u;
    out.clear();
    out.reserve(kWebpRiffBytes + len + pad);
    auto put_le32 = [&](uint64_t v) {
        for (int k = 0; k < 4; ++k) out.push_back((uint8_t)(v >> (8 * k)));
    };
    out.insert(out.end(), {'R', 'I', 'F', 'F'});
    put_le32(4 + 8 + len + pad);
    out.insert(out.end(), {'W', 'E', 'B', 'P', 'V', 'P', '8', 'L'});
    put_le32(len);
    out.insert(out.end(), payload, payload + len);
    if (pad) out.push_back(0);
}

bool encode_webp(const uint8_t* rgba, int W, int H, int C, std::vector<uint8_t>& out) {
    const uint64_t bound = webp_body_max_bytes(W, H, C);
    if (!rgba || bound == 0) return false;
    const size_t n = (size_t)W * (size_t)H;
    std::vector<uint32_t> resid(n);
    auto pixel = [&](size_t i) {
        uint32_t v;
        std::memcpy(&v, rgba + 4 * i, 4);  // little-endian host: R in the low byte
        return webp_pixel(v, C);
    };
    for (size_t i = 0; i < n; ++i) {
        const uint32_t pred = i % (size_t)W ? pixel(i - 1) : i ? pixel(i - (size_t)W) : kWebpFirstPrediction;
        resid[i] = webp_sub(pixel(i), pred);
    }
    // the rule as a plain walk over the rows' stretches: lit(residual), copy(length)
    auto walk = [&](auto&& lit, auto&& copy) {
        for (int y = 0; y < H; ++y) {
            const uint32_t* row = resid.data() + (size_t)y * (size_t)W;
            for (int x = 0; x < W;) {
                if (x == 0 || row[x] != row[x - 1]) {
                    lit(row[x++]);
                    continue;
                }
                int e = x + 1;  // the stretch [x, e)
                while (e < W && row[e] == row[e - 1]) ++e;
                while (x < e) {
                    const uint32_t m = std::min<uint32_t>(kWebpMaxCopy, (uint32_t)(e - x));
                    if (m >= kWebpMinRun) copy(m);
                    else
                        for (uint32_t k = 0; k < m; ++k) lit(row[x + (int)k]);
                    x += (int)m;
                }
            }
        }
    };
    std::vector<uint32_t> freq((size_t)kWebpSyms, 0u), codes((size_t)kWebpSyms, 0u);
    walk(
        [&](uint32_t v) {
            freq[(size_t)kWebpGreen + ((v >> 8) & 255u)] += 1u;
            freq[(size_t)kWebpRed + ((v >> 16) & 255u)] += 1u;
            freq[(size_t)kWebpBlue + (v & 255u)] += 1u;
            freq[(size_t)kWebpAlpha + (v >> 24)] += 1u;
        },
        [&](uint32_t len) {
            uint32_t sym, nb, extra;
            webp_prefix(len, sym, nb, extra);
            freq[(size_t)kWebpGreen + 256 + sym] += 1u;
            freq[(size_t)kWebpDist + kWebpDistSym] += 1u;
        });
    std::vector<uint8_t> body;
    WebpBits b{body};
    b.put(0x2Fu, 8);
    b.put((uint32_t)(W - 1), 14);
    b.put((uint32_t)(H - 1), 14);
    b.put(C == 4 ? 1u : 0u, 1);  // alpha_is_used
    b.put(0u, 3);                // version
    b.put(1u, 1), b.put(2u, 2);  // a transform: subtract-green
    b.put(1u, 1), b.put(0u, 2);  // a transform: predictor
    b.put(kWebpBlockBits - 2u, 3);
    b.put(0u, 1);                // its sub-image: no colour cache
    b.simple(1, 1u, 0u);         // green: mode 1 in every block
    for (int a = 1; a < kWebpAlphabets; ++a) b.simple(1, 0u, 0u);
    b.put(0u, 1);                // no more transforms
    b.put(0u, 1), b.put(0u, 1);  // the image: no colour cache, no meta prefix codes
    for (int a = 0; a < kWebpAlphabets; ++a)
        webp_write_code(b, freq.data() + webp_base(a), webp_size(a), codes.data() + webp_base(a));
    auto code = [&](size_t s) { b.put(codes[s] & 0xFFFFu, (int)(codes[s] >> 16)); };
    walk(
        [&](uint32_t v) {
            code((size_t)kWebpGreen + ((v >> 8) & 255u));
            code((size_t)kWebpRed + ((v >> 16) & 255u));
            code((size_t)kWebpBlue + (v & 255u));
            code((size_t)kWebpAlpha + (v >> 24));
        },
        [&](uint32_t len) {
            uint32_t sym, nb, extra;
            webp_prefix(len, sym, nb, extra);
            code((size_t)kWebpGreen + 256 + sym);
            b.put(extra, (int)nb);
            code((size_t)kWebpDist + kWebpDistSym);
        });
    b.flush();
    webp_wrap_stream(body.data(), body.size(), out);
    return body.size() <= bound;
}

bool write_file(const std::string& path, const std::vector<uint8_t>& data) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const size_t n = std::fwrite(data.data(), 1, data.size(), f);
    const bool ok = n == data.size() && std::fclose(f) == 0;
    if (n != data.size()) std::fclose(f);
    return ok;
}

}  // namespace rr
