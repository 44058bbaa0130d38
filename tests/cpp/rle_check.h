// What the stand-alone checks of the run-length coders (tga_check.cpp,
// hdr_check.cpp, iris_check.cpp) share, over a format's traits T
// (csrc/rle_rule.h): the lane-at-a-time walk of the device packer, and the
// comparison of the generic window functions with a format's closed form.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

#include "rle_rule.h"

// One row's packets from the eq bits and the rule's window functions, an
// element ("lane") at a time as rle_device.hpp rle_pack_row forms them. p: the
// row's elements, T::kElemBytes bytes each.
template <class T>
void pack_by_windows(const std::vector<uint8_t>& p, std::vector<uint8_t>& out) {
    constexpr size_t c = T::kElemBytes;
    const int W = (int)(p.size() / c);
    auto eq = [&](int j) { return j > 0 && j < W && std::memcmp(&p[c * (size_t)j], &p[c * (size_t)(j - 1)], c) == 0; };
    int first = 0;
    for (int i = 0; i < W; ++i) {
        uint32_t win = 0;  // bit k: eq(i - 3 + k)
        for (int k = 0; k < 8; ++k) win |= (uint32_t)eq(i - 3 + k) << k;
        const bool run = rr::rle_in_run<T>(win >> 1);
        const bool start = i == 0 || rr::rle_stretch_start<T>(win);
        const bool next_starts = i + 1 >= W || rr::rle_stretch_start<T>(win >> 1);
        if (start) first = i;
        const uint32_t cap = rr::rle_packet_cap<T>(run);
        const uint32_t q = (uint32_t)(i - first) % cap;
        if (q == cap - 1u || next_starts) {  // a packet's last element knows its count
            out.push_back((uint8_t)T::header(run, q + 1u));
            const size_t from = run ? (size_t)i : (size_t)i - q;
            out.insert(out.end(), p.data() + c * from, p.data() + c * ((size_t)i + 1));
        }
    }
}

// Over all 256 eight-bit windows (bit k: eq(i - 3 + k)): how many times T's
// generic rle_in_run and rle_stretch_start, for element i and for i + 1 as the
// packer asks them, differ from the format's closed form. in_run(eq): whether
// an element is in a run stretch, eq(d) being the eq bit d elements after its
// own, as the format's rule comment writes it out.
template <class T, class InRun>
int window_mismatches(InRun in_run) {
    int bad = 0;
    for (uint32_t win = 0; win < 256u; ++win) {
        // element i + o: its kind, and whether a stretch starts at it (when it is not element 0)
        auto kind = [&](int o) { return (bool)in_run([&](int d) { return (bool)((win >> (3 + o + d)) & 1u); }); };
        auto starts = [&](int o) { return kind(o) != kind(o - 1) || (kind(o) && !((win >> (3 + o)) & 1u)); };
        bad += rr::rle_in_run<T>(win >> 1) != kind(0);
        bad += rr::rle_stretch_start<T>(win) != starts(0);
        bad += rr::rle_stretch_start<T>(win >> 1) != starts(1);
    }
    return bad;
}
