// Host image encoders (see image_io.cpp).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace rr {

int encoder_threads();

// Baseline JPEG tables for a quality: quantisers (natural order), their
// reciprocals, and the 8x8 DCT basis c[u][x] = C(u)/2 cos((2x+1) u pi / 16).
struct JpegTables {
    uint8_t ql[64], qc[64];
    float qinv_l[64], qinv_c[64];
    float dct[64];
};
void jpeg_tables(int quality, JpegTables& t);
// Quantised coefficients of a whole image: [mcuy][mcux][6 blocks][64], natural
// order, blocks Y00 Y01 Y10 Y11 Cb Cr (4:2:0, edge-replicated padding).
// grey: a one-component file, [mcuy][mcux][64] with MCUs of 8x8 pixels.
size_t jpeg_coeff_count(int W, int H, bool grey = false);
bool encode_jpeg_coeffs(const int16_t* coeffs, int W, int H, int quality, std::vector<uint8_t>& out,
                        int threads = 0);
// The file bytes in front of the entropy-coded segment (SOI ... SOS), and the
// Huffman tables as 4 x 256 packed code | len << 16 (DC luma, AC luma, DC
// chroma, AC chroma) for the device coder (jpeg.hip).
void jpeg_header_bytes(int W, int H, int quality, std::vector<uint8_t>& out, bool grey = false);
void jpeg_huff_tables(uint32_t out[4 * 256]);
// grey: single-component baseline (SOF0 with one component 1x1, the luma DQT
// and DHT pair), Y the pixel's grey code (grey.h), restart interval one row of
// 8x8 MCUs; jpeg.hip writes the same bytes.
bool encode_jpeg(const uint8_t* rgba, int W, int H, int quality, std::vector<uint8_t>& out, int threads = 0,
                 bool grey = false);
// channels: what the file holds of the RGBA8 image: 4 RGBA (colour type 6), 3
// RGB (2), 1 the grey code of grey.h (0). level: zlib's, 0 (stored blocks) to
// 9. adaptive: every row takes libpng's adaptive filter (png_filter.h), against
// the image's row above whatever the thread bands; false: Sub on every row.
bool encode_png(const uint8_t* rgba, int W, int H, std::vector<uint8_t>& out, int level = 1, int threads = 0,
                int channels = 4, bool adaptive = false);
// zlib's level of Blender's image_settings.compression (0 .. 100):
// (int)(compression / 11.1111f), clamped to 0 .. 9.
int png_zlib_level(int compression);
// The PNG file around a zlib stream coded on the device (png.hip): z = 78 01 +
// the bands' deflate pieces; band_tab = {Adler-32, filtered bytes} per band,
// combined here into the stream's Adler-32. Signature, IHDR, one IDAT, IEND.
// depth: bits per sample of the RGBA image the stream holds, 8 (png.hip) or 16
// (png16.hip: big-endian samples, rows of 8W + 1 filtered bytes). color_type:
// 6 RGBA, 2 RGB, 0 grey, as the stream's rows were formed.
void png_wrap_stream(int W, int H, const uint8_t* z, size_t n, const uint32_t* band_tab, int nbands,
                     std::vector<uint8_t>& out, int depth = 8, int color_type = 6);
// The OpenEXR file (single-part scanline, version 2; half A, B, G, R; ZIP,
// chunks of 16 scanlines) around chunks coded on the device (exr.hip): data =
// the chunks' pieces back to back, chunk_tab = {mode, bytes, Adler-32, chunk
// bytes} per chunk. Mode 0: deflate data, wrapped here in 78 01 ... Adler-32;
// mode 1: the raw chunk. pixel_type: 1 HALF (8W bytes a scanline) or 2 FLOAT
// (16W), the type of all four channels; nothing else in the header depends on
// it. compression: the header's attribute, 3 ZIP or 5 PXR24 (whose FLOAT
// chunks code 3 bytes a sample; a raw chunk is the full floats). channels: 4 the list A, B, G, R; 3: B, G, R; 1: Y. false: the pieces do
// not add up to n, or a chunk's size is not what its scanlines allow.
bool exr_wrap_stream(int W, int H, const uint8_t* data, size_t n, const uint32_t* chunk_tab, int nchunks,
                     std::vector<uint8_t>& out, int pixel_type = 1, int channels = 4, int compression = 3);
// The same file with a chunk per scanline (compression 0 NONE, 1 RLE) around
// the dense body coded on the device (exr_codec.hip): data = the scanlines'
// chunks back to back, row_tab = {mode, bytes} per scanline, mode 0 packets
// (fewer bytes than the scanline's), 1 the raw scanline; nullptr: every
// scanline raw. false: the chunks do not add up to n, or a size is not what
// its scanline allows.
bool exr_wrap_rows(int W, int H, const uint8_t* data, size_t n, const uint32_t* row_tab, std::vector<uint8_t>& out,
                   int pixel_type, int channels, int compression);
// The packets of an RLE chunk for n bytes already reordered and differenced,
// appended to out: the host statement of exr_rle_rule.h.
void exr_rle_pack(const uint8_t* bytes, size_t n, std::vector<uint8_t>& out);
// A TARGA file of the RGBA8 image (tga_rule.h): the 18-byte header (no id, no
// colour map, type 2 true colour or 3 grey, + 8 run-length coded, bottom-left
// origin, 8 C bits a pixel, 8 alpha bits for C = 4) and the body, rows bottom
// first, pixels B, G, R(, A) or the grey code of grey.h; rle: packets by the
// rule of tga_rule.h ("TARGA"), else the plain bytes ("TARGA_RAW"). No footer.
// false: W or H above 65535, C not 1, 3 or 4, or a body of 2 GB and more.
// tga.hip writes the same bytes.
bool encode_tga(const uint8_t* rgba, int W, int H, int C, bool rle, std::vector<uint8_t>& out);
void tga_header_bytes(int W, int H, int C, bool rle, std::vector<uint8_t>& out);
// A Radiance RGBE file ("HDR") of W x H float RGBA means (alpha ignored), by
// the rules of hdr_rule.h: the text header "#?RADIANCE\nFORMAT=32-bit_rle_rgbe
// \n\n-Y <H> +X <W>\n" and the rows top first, each the marker bytes and the
// four planes in packets, or flat quads where the width says so. C = 3: the
// quads of R, G, B; C = 1: of the Rec.709 luma (grey.h luma709) in all three.
// The rule is stated as a plain walk over the runs: hdr.hip writes the same
// bytes from ballots. false: C not 1 or 3, or a body bound of 2 GB and more.
bool encode_hdr(const float* rgba, int W, int H, int C, std::vector<uint8_t>& out);
void hdr_header_bytes(int W, int H, std::vector<uint8_t>& out);
// A Silicon Graphics image file ("IRIS", .rgb) of the RGBA8 image, by the rules
// of iris_rule.h, every number big-endian: the 512-byte header (magic 474,
// run-length coded, a byte a channel, dimension 2 for C = 1 else 3, W, H, C,
// pixmin 0, pixmax 255, no name, colour map id 0), the start and the length
// table, and the row-planes in packets, rows bottom first, channels R, G, B(, A)
// or the grey code of grey.h. The rule is stated as a plain walk over the runs:
// iris.hip writes the same bytes from ballots. false: W or H above 65535, C not
// 1, 3 or 4, or a body bound of 2 GB and more.
bool encode_iris(const uint8_t* rgba, int W, int H, int C, std::vector<uint8_t>& out);
void iris_header_bytes(int W, int H, int C, std::vector<uint8_t>& out);
// A lossless WebP file ("WEBP", .webp) of the RGBA8 image, by the rules of
// webp_rule.h: a RIFF container with one VP8L chunk, subtract-green, the
// left-neighbour predictor, copies at distance 1 of at least kWebpMinRun equal
// residuals, five prefix codes. C = 4: the pixels as they are, alpha hint 1;
// C = 3: alpha 255, hint 0; C = 1: the grey code of grey.h in R, G and B. The
// rule is stated as a plain walk over the stretches: webp.hip writes the same
// bytes from ballots and scans. false: W or H outside 1 .. 16384, C not 1, 3 or
// 4, or a payload bound of 2 GB and more.
bool encode_webp(const uint8_t* rgba, int W, int H, int C, std::vector<uint8_t>& out);
// The file around a VP8L payload: "RIFF", the size, "WEBP", "VP8L", the
// payload's size, the payload, and a 0 byte if its size is odd.
void webp_wrap_stream(const uint8_t* payload, size_t len, std::vector<uint8_t>& out);
bool write_file(const std::string& path, const std::vector<uint8_t>& data);

}  // namespace rr
