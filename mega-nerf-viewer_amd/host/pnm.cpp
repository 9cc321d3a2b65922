// pnm.cpp -- mnv_pnm_read: binary PNM files (P6 / P5, maxval 255) for the targets and masks of `mnv_render --target`.  The header is parsed
// from a bounded buffer, every index is checked against what was read; the contract is stated in include/mnv.h.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mnv.h"
#include "../csrc/mnv_error.h"

namespace {

// the header of a PNM file is a few dozen bytes; comments may make it longer, 64 KiB is far beyond any writer's
constexpr size_t kMaxHeader = 65536;

struct Cursor {
    const std::vector<uint8_t> &buf;
    size_t at = 0;
    bool is_space(uint8_t c) const { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\v' || c == '\f'; }
    // skip white space and `#` comments (to the end of the line); false at the end of the buffer
    bool skip_blank() {
        while (at < buf.size()) {
            if (buf[at] == '#') {
                while (at < buf.size() && buf[at] != '\n') ++at;
            } else if (is_space(buf[at])) {
                ++at;
            } else {
                return true;
            }
        }
        return false;
    }
    // a decimal number of at most 9 digits; false when there is none, or when the buffer ends inside it
    bool number(int64_t *out) {
        if (!skip_blank()) return false;
        int64_t v = 0;
        int digits = 0;
        while (at < buf.size() && buf[at] >= '0' && buf[at] <= '9') {
            if (++digits > 9) return false;
            v = v * 10 + (buf[at] - '0');
            ++at;
        }
        if (digits == 0 || at >= buf.size()) return false;
        *out = v;
        return true;
    }
};

}  // namespace

extern "C" int mnv_pnm_read(const char *path, int32_t expect_width, int32_t expect_height, uint8_t *data, int64_t cap_bytes, int32_t *width,
                            int32_t *height, int32_t *channels) {
    if (width) *width = 0;
    if (height) *height = 0;
    if (channels) *channels = 0;
    if (!path) return mnv::set_error(MNV_E_INVALID, "mnv_pnm_read: null path");
    if (cap_bytes < 0 || (cap_bytes > 0 && !data)) return mnv::set_error(MNV_E_INVALID, "mnv_pnm_read: invalid output buffer");
    const std::string name(path);
    std::FILE *fp = std::fopen(path, "rb");
    if (!fp) return mnv::set_error(MNV_E_IO, ("mnv_pnm_read: cannot open " + name).c_str());
    std::vector<uint8_t> head(kMaxHeader);
    head.resize(std::fread(head.data(), 1, head.size(), fp));
    auto fail = [&](int code, const std::string &what) {
        std::fclose(fp);
        return mnv::set_error(code, ("mnv_pnm_read: " + name + ": " + what).c_str());
    };
    if (head.size() < 2 || head[0] != 'P' || (head[1] != '6' && head[1] != '5')) return fail(MNV_E_IO, "not a binary PPM (P6) or PGM (P5) file");
    const int ch = head[1] == '6' ? 3 : 1;
    Cursor cur{head, 2};
    int64_t w = 0, h = 0, maxval = 0;
    if (!cur.number(&w) || !cur.number(&h) || !cur.number(&maxval)) return fail(MNV_E_IO, "malformed or truncated header");
    // exactly one white-space byte separates the header from the data (number() left the cursor on a byte inside the buffer)
    if (!cur.is_space(head[cur.at])) return fail(MNV_E_IO, "malformed header");
    const size_t data_at = cur.at + 1;
    if (w < 1 || h < 1 || w * h > ((int64_t)1 << 28)) return fail(MNV_E_IO, "an image of " + std::to_string(w) + " x " + std::to_string(h) + " pixels");
    if (maxval != 255) return fail(MNV_E_IO, "maxval " + std::to_string(maxval) + " (only 255 is read)");
    if (width) *width = (int32_t)w;
    if (height) *height = (int32_t)h;
    if (channels) *channels = ch;
    if ((expect_width > 0 && w != expect_width) || (expect_height > 0 && h != expect_height))
        return fail(MNV_E_IO, "the image is " + std::to_string(w) + " x " + std::to_string(h) + ", expected " + std::to_string(expect_width) + " x " +
                                  std::to_string(expect_height));
    const int64_t need = w * h * ch;
    if (!data) {  // the size query; the data must still be there
        if (std::fseek(fp, 0, SEEK_END) != 0 || std::ftell(fp) < (long)(data_at + (size_t)need)) return fail(MNV_E_IO, "fewer data bytes than the header promises");
        std::fclose(fp);
        return MNV_OK;
    }
    if (cap_bytes < need) return fail(MNV_E_INVALID, "buffer too small (width * height * channels bytes are needed)");
    // the part of the data that came with the header block, then the rest
    const size_t have = head.size() > data_at ? std::min<size_t>(head.size() - data_at, (size_t)need) : 0;
    if (have) std::memcpy(data, head.data() + data_at, have);
    if (have < (size_t)need && std::fread(data + have, 1, (size_t)need - have, fp) != (size_t)need - have)
        return fail(MNV_E_IO, "fewer data bytes than the header promises");
    std::fclose(fp);
    return MNV_OK;
}
