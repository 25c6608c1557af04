// Readers of HDR environment maps, beside png_read.hpp: Radiance .hdr (RGBE; flat and new-style run-length scanlines,
// "-Y H +X W" orientation) and PFM ("PF": three fp32 per pixel, rows bottom to top, endianness from the sign of the scale
// line).  Both decode a file held in memory and never read past it; rows x cols is checked against max_texels before any
// pixel is decoded.  -> RT_OK, RT_ERR_SCENE (malformed), RT_ERR_IO (truncated) or RT_ERR_LIMIT, with a message in err.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rtmi.h"

namespace rtmi {
namespace envfile {

inline bool is_hdr(const std::vector<uint8_t> &f) { return f.size() >= 2 && f[0] == '#' && f[1] == '?'; }
inline bool is_pfm(const std::vector<uint8_t> &f) {
    return f.size() >= 3 && f[0] == 'P' && (f[1] == 'F' || f[1] == 'f') && (f[2] == '\n' || f[2] == ' ' || f[2] == '\r' || f[2] == '\t');
}

// one header line (without its '\n'); false at the end of the file
inline bool line(const std::vector<uint8_t> &f, size_t &pos, std::string &out) {
    out.clear();
    if (pos >= f.size()) return false;
    while (pos < f.size() && f[pos] != '\n') {
        if (out.size() > 4096) return false;
        out.push_back((char)f[pos++]);
    }
    if (pos >= f.size()) return false;  // a header line ends with a newline
    ++pos;
    if (!out.empty() && out.back() == '\r') out.pop_back();
    return true;
}

inline int check_size(long long rows, long long cols, long long max_texels, std::string &err) {
    if (rows < 1 || cols < 1 || rows > (1LL << 30) || cols > (1LL << 30)) {
        err = "bad image size";
        return RT_ERR_SCENE;
    }
    if (rows * cols > max_texels) {
        err = "environment map of " + std::to_string(rows) + " x " + std::to_string(cols) + " texels exceeds the limit of " +
              std::to_string(max_texels);
        return RT_ERR_LIMIT;
    }
    return RT_OK;
}

inline int read_hdr(const std::vector<uint8_t> &f, long long max_texels, int &rows, int &cols, std::vector<float> &rgb, std::string &err) {
    size_t pos = 0;
    std::string ln;
    if (!line(f, pos, ln) || (ln != "#?RADIANCE" && ln != "#?RGBE")) {
        err = "not a Radiance file (#?RADIANCE)";
        return RT_ERR_SCENE;
    }
    bool format_ok = false;
    for (;;) {
        if (!line(f, pos, ln)) {
            err = "header without an end";
            return RT_ERR_SCENE;
        }
        if (ln.empty()) break;
        if (ln.compare(0, 7, "FORMAT=") == 0) {
            if (ln != "FORMAT=32-bit_rle_rgbe") {
                err = "unsupported " + ln + " (32-bit_rle_rgbe only)";
                return RT_ERR_SCENE;
            }
            format_ok = true;
        }
    }
    if (!format_ok) {
        err = "header without FORMAT=32-bit_rle_rgbe";
        return RT_ERR_SCENE;
    }
    long long h = 0, w = 0;
    char tail = 0;
    if (!line(f, pos, ln) || sscanf(ln.c_str(), "-Y %lld +X %lld%c", &h, &w, &tail) != 2) {
        err = "resolution line must be \"-Y H +X W\"";
        return RT_ERR_SCENE;
    }
    int rc = check_size(h, w, max_texels, err);
    if (rc) return rc;
    rows = (int)h, cols = (int)w;
    rgb.assign((size_t)h * (size_t)w * 3, 0.0f);
    std::vector<uint8_t> scan((size_t)w * 4);
    for (long long y = 0; y < h; ++y) {
        const bool rle = w >= 8 && w <= 32767 && f.size() - pos >= 4 && f[pos] == 2 && f[pos + 1] == 2 && (f[pos + 2] & 0x80) == 0;
        if (rle) {
            if (((long long)f[pos + 2] << 8 | f[pos + 3]) != w) {
                err = "run-length scanline of another width";
                return RT_ERR_SCENE;
            }
            pos += 4;
            for (int ch = 0; ch < 4; ++ch) {
                long long x = 0;
                while (x < w) {
                    if (pos >= f.size()) {
                        err = "truncated";
                        return RT_ERR_IO;
                    }
                    int n = f[pos++];
                    if (n > 128) {  // a run
                        n -= 128;
                        if (pos >= f.size()) {
                            err = "truncated";
                            return RT_ERR_IO;
                        }
                        if (x + n > w) {
                            err = "run past the end of a scanline";
                            return RT_ERR_SCENE;
                        }
                        const uint8_t v = f[pos++];
                        for (int k = 0; k < n; ++k) scan[(size_t)(x + k) * 4 + ch] = v;
                    } else {  // literals
                        if (n == 0 || x + n > w) {
                            err = "bad literal count in a scanline";
                            return RT_ERR_SCENE;
                        }
                        if (f.size() - pos < (size_t)n) {
                            err = "truncated";
                            return RT_ERR_IO;
                        }
                        for (int k = 0; k < n; ++k) scan[(size_t)(x + k) * 4 + ch] = f[pos++];
                    }
                    x += n;
                }
            }
        } else {
            if (f.size() - pos < (size_t)w * 4) {
                err = "truncated";
                return RT_ERR_IO;
            }
            memcpy(scan.data(), f.data() + pos, (size_t)w * 4);
            pos += (size_t)w * 4;
        }
        float *dst = rgb.data() + (size_t)y * (size_t)w * 3;
        for (long long x = 0; x < w; ++x) {
            const uint8_t *q = scan.data() + (size_t)x * 4;
            if (q[3] == 0) continue;  // (zeros)
            const float sc = std::ldexp(1.0f, (int)q[3] - 136);  // mantissa x 2^(e - 128 - 8)
            dst[3 * x] = (float)q[0] * sc, dst[3 * x + 1] = (float)q[1] * sc, dst[3 * x + 2] = (float)q[2] * sc;
        }
    }
    return RT_OK;
}

inline int read_pfm(const std::vector<uint8_t> &f, long long max_texels, int &rows, int &cols, std::vector<float> &rgb, std::string &err) {
    if (f.size() < 3 || f[0] != 'P' || f[1] != 'F') {
        err = "not a colour PFM file (PF)";
        return RT_ERR_SCENE;
    }
    // three whitespace-separated tokens after the magic, then ONE whitespace byte, then the data
    size_t pos = 2;
    std::string tok[3];
    for (int k = 0; k < 3; ++k) {
        while (pos < f.size() && (f[pos] == ' ' || f[pos] == '\n' || f[pos] == '\r' || f[pos] == '\t')) ++pos;
        while (pos < f.size() && !(f[pos] == ' ' || f[pos] == '\n' || f[pos] == '\r' || f[pos] == '\t') && tok[k].size() < 64) tok[k].push_back((char)f[pos++]);
        if (tok[k].empty()) {
            err = "PFM header: width, height and scale expected";
            return RT_ERR_SCENE;
        }
    }
    char *end = nullptr;
    const long long w = strtoll(tok[0].c_str(), &end, 10);
    const bool w_ok = *end == 0;
    const long long h = strtoll(tok[1].c_str(), &end, 10);
    const bool h_ok = *end == 0;
    const double scale = strtod(tok[2].c_str(), &end);
    if (!w_ok || !h_ok || *end != 0 || !(scale != 0.0) || !std::isfinite(scale)) {
        err = "PFM header: width, height and a nonzero scale expected";
        return RT_ERR_SCENE;
    }
    int rc = check_size(h, w, max_texels, err);
    if (rc) return rc;
    if (pos >= f.size()) {
        err = "truncated";
        return RT_ERR_IO;
    }
    ++pos;
    const size_t n = (size_t)h * (size_t)w * 3;
    if ((f.size() - pos) / 4 < n) {
        err = "truncated";
        return RT_ERR_IO;
    }
    rows = (int)h, cols = (int)w;
    rgb.resize(n);
    const bool little = scale < 0.0;
    const float mul = (float)std::fabs(scale);
    const size_t row_floats = (size_t)w * 3;
    for (long long y = 0; y < h; ++y) {  // the file's first row is the image's bottom row
        const uint8_t *src = f.data() + pos + (size_t)(h - 1 - y) * row_floats * 4;
        float *dst = rgb.data() + (size_t)y * row_floats;
        for (size_t i = 0; i < row_floats; ++i) {
            const uint8_t *b = src + 4 * i;
            const uint32_t u = little ? ((uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24)
                                      : ((uint32_t)b[3] | (uint32_t)b[2] << 8 | (uint32_t)b[1] << 16 | (uint32_t)b[0] << 24);
            float v;
            memcpy(&v, &u, 4);
            dst[i] = v * mul;
        }
    }
    return RT_OK;
}

}  // namespace envfile
}  // namespace rtmi
