// srcnnyuv -- YUV4MPEG2 (.y4m) video through srcnn_yuv420_upscale_dev (include/srcnn_amd_yuv.h) or, with --all-formats,
// srcnn_yuv_upscale_dev (include/srcnn_amd_yuv_ex.h): every frame's Y plane goes through SRCNN with the chosen filter, its
// chroma planes through the chroma filter, and the result is written as a YUV4MPEG2 stream again.
//
//   srcnnyuv [--all-formats] [--scale M] [--filter nearest|bilinear|bicubic|lanczos3|bspline] IN.y4m|- OUT.y4m|-
//
// Input: 8-bit 4:2:0 (C420, C420jpeg, C420paldv, C420mpeg2, or no C tag), progressive (Ip or no I tag).  Every other colour
// space, every bit depth above 8 and interlaced input are refused with exit status 2 and a one-line message, before the
// device is touched.  --all-formats also takes C422 and C444 and the p10 / p12 / p14 / p16 forms of C420, C422 and C444
// (YUV4MPEG2 stores those planar, little-endian, value in the low bits); mono, alpha, any other depth and interlaced streams
// are still refused with status 2.  The output header is the input's with W and H replaced; every other tag and every frame's parameters
// are copied verbatim.  Frames move through two page-locked staging slots on two streams, so that the upload of frame i+1
// overlaps the kernels of frame i.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/srcnn_amd.h"
#include "../include/srcnn_amd_yuv.h"
#include "../include/srcnn_amd_yuv_ex.h"

namespace {

[[noreturn]] void die(int status, const char* fmt, const char* arg = "")
{
    std::fprintf(stderr, "srcnnyuv: ");
    std::fprintf(stderr, fmt, arg);
    std::fprintf(stderr, "\n");
    std::exit(status);
}

void usage()
{
    std::fprintf(stderr, "usage: srcnnyuv [--all-formats] [--scale M] [--filter nearest|bilinear|bicubic|lanczos3|bspline] IN.y4m|- OUT.y4m|-\n");
    std::exit(2);
}

// one header or FRAME line without its '\n'; false at a clean end of file
bool read_line(FILE* f, std::string& line)
{
    line.clear();
    int c;
    while ((c = std::fgetc(f)) != EOF) {
        if (c == '\n') return true;
        line.push_back((char)c);
        if (line.size() > 4096) die(2, "header line too long");
    }
    if (!line.empty()) die(2, "truncated line at end of input");
    return false;
}

std::vector<std::string> split(const std::string& s)
{
    std::vector<std::string> out;
    size_t a = 0;
    while (a < s.size()) {
        size_t b = s.find(' ', a);
        if (b == std::string::npos) b = s.size();
        if (b > a) out.push_back(s.substr(a, b - a));
        a = b + 1;
    }
    return out;
}

struct Slot {
    void* stream = nullptr;
    unsigned char* pin_in = nullptr;
    unsigned char* pin_out = nullptr;
    unsigned char* d_in = nullptr;
    unsigned char* d_out = nullptr;
    std::string params;                 // the FRAME line's parameters, copied verbatim
    bool pending = false;
};

// "C420p10" -> (SRCNN_YUV_420, 10); false for what --all-formats does not take (mono, alpha, 411, other depths)
bool parse_colour_space(const std::string& tag, int& chroma, int& depth)
{
    std::string t = tag.substr(1);
    depth = 8;
    const size_t p = t.find('p', 3);
    if (t.compare(0, 3, "420") == 0 && (t == "420" || t == "420jpeg" || t == "420paldv" || t == "420mpeg2")) { chroma = SRCNN_YUV_420; return true; }
    if (t == "422") { chroma = SRCNN_YUV_422; return true; }
    if (t == "444") { chroma = SRCNN_YUV_444; return true; }
    if (p != 3) return false;
    const std::string base = t.substr(0, 3), d = t.substr(4);
    if (base == "420") chroma = SRCNN_YUV_420;
    else if (base == "422") chroma = SRCNN_YUV_422;
    else if (base == "444") chroma = SRCNN_YUV_444;
    else return false;
    if (d == "10") depth = 10;
    else if (d == "12") depth = 12;
    else if (d == "14") depth = 14;
    else if (d == "16") depth = 16;
    else return false;
    return true;
}

void check(int rc, const char* what)
{
    if (rc != SRCNN_OK) {
        std::fprintf(stderr, "srcnnyuv: %s failed (%d): %s\n", what, rc, srcnn_last_error());
        std::exit(1);
    }
}

}  // namespace

int main(int argc, char** argv)
{
    float scale = 2.0f;
    int filter = SRCNN_FILTER_BICUBIC;
    bool all_formats = false;
    std::vector<const char*> files;
    static const char* const kFilters[] = {"nearest", "bilinear", "bicubic", "lanczos3", "bspline"};
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--scale" && i + 1 < argc) {
            char* end = nullptr;
            scale = std::strtof(argv[++i], &end);
            if (!end || *end || !(scale > 0.f)) die(2, "bad --scale %s", argv[i]);
        } else if (a == "--filter" && i + 1 < argc) {
            const std::string v = argv[++i];
            filter = -1;
            for (int k = 0; k < 5; ++k)
                if (v == kFilters[k]) filter = k;
            if (filter < 0) die(2, "unknown filter %s", v.c_str());
        } else if (a == "--all-formats") {
            all_formats = true;
        } else if (a == "-h" || a == "--help") {
            usage();
        } else if (a.size() > 1 && a[0] == '-' && a != "-") {
            die(2, "unknown option %s", a.c_str());
        } else {
            files.push_back(argv[i]);
        }
    }
    if (files.size() != 2) usage();
    FILE* in = std::strcmp(files[0], "-") == 0 ? stdin : std::fopen(files[0], "rb");
    if (!in) die(2, "cannot open %s", files[0]);

    // ---- header: validated completely before the device is touched ----
    std::string line;
    if (!read_line(in, line)) die(2, "empty input");
    std::vector<std::string> tags = split(line);
    if (tags.empty() || tags[0] != "YUV4MPEG2") die(2, "not a YUV4MPEG2 stream");
    unsigned w = 0, h = 0;
    srcnn_yuv_format fmt = {(unsigned)sizeof(srcnn_yuv_format), SRCNN_YUV_PLANAR, SRCNN_YUV_420, 8, 0};
    for (size_t k = 1; k < tags.size(); ++k) {
        const std::string& t = tags[k];
        if (t[0] == 'W') w = (unsigned)std::strtoul(t.c_str() + 1, nullptr, 10);
        else if (t[0] == 'H') h = (unsigned)std::strtoul(t.c_str() + 1, nullptr, 10);
        else if (t[0] == 'C' && all_formats) {
            if (!parse_colour_space(t, fmt.chroma, fmt.depth))
                die(2, "unsupported colour space %s (4:2:0 / 4:2:2 / 4:4:4 at 8, 10, 12, 14 or 16 bits only)", t.c_str());
        } else if (t[0] == 'C' && t != "C420" && t != "C420jpeg" && t != "C420paldv" && t != "C420mpeg2")
            die(2, "unsupported colour space %s (8-bit 4:2:0 only)", t.c_str());
        else if (t[0] == 'I' && t != "Ip") die(2, "unsupported interlacing %s (progressive only)", t.c_str());
    }
    if (w == 0 || h == 0) die(2, "missing or zero W / H");
    unsigned dw = 0, dh = 0;
    if (srcnn_output_size(w, h, scale, 0, &dw, &dh) != SRCNN_OK) die(2, "--scale gives an empty frame");
    // tight planes, one after the other: [0] = Y bytes, [1] = bytes of one chroma plane
    size_t in_plane[2], out_plane[2];
    for (int k = 0; k < 2; ++k) {
        unsigned rows = 0;
        size_t rb = 0;
        if (srcnn_yuv_plane_size(&fmt, w, h, k, nullptr, &rows, &rb) != SRCNN_OK) die(2, "%s", srcnn_last_error());
        in_plane[k] = rb * rows;
        if (srcnn_yuv_plane_size(&fmt, dw, dh, k, nullptr, &rows, &rb) != SRCNN_OK) die(2, "%s", srcnn_last_error());
        out_plane[k] = rb * rows;
    }
    const size_t in_bytes = in_plane[0] + 2 * in_plane[1], out_bytes = out_plane[0] + 2 * out_plane[1];

    FILE* out = std::strcmp(files[1], "-") == 0 ? stdout : std::fopen(files[1], "wb");
    if (!out) die(2, "cannot create %s", files[1]);
    std::string hdr = "YUV4MPEG2";
    for (size_t k = 1; k < tags.size(); ++k) {
        if (tags[k][0] == 'W') hdr += " W" + std::to_string(dw);
        else if (tags[k][0] == 'H') hdr += " H" + std::to_string(dh);
        else hdr += " " + tags[k];
    }
    hdr += "\n";
    if (std::fwrite(hdr.data(), 1, hdr.size(), out) != hdr.size()) die(1, "write error");

    // ---- two slots: frame i+1's upload (its slot's stream) overlaps frame i's kernels (the other stream) ----
    Slot slots[2];
    for (Slot& s : slots) {
        check(srcnn_stream_create(&s.stream), "srcnn_stream_create");
        s.pin_in = (unsigned char*)srcnn_host_alloc_pinned(in_bytes);
        s.pin_out = (unsigned char*)srcnn_host_alloc_pinned(out_bytes);
        s.d_in = (unsigned char*)srcnn_dev_alloc(in_bytes);
        s.d_out = (unsigned char*)srcnn_dev_alloc(out_bytes);
        if (!s.pin_in || !s.pin_out || !s.d_in || !s.d_out) check(SRCNN_E_DEVMEM, "allocation");
    }
    auto flush = [&](Slot& s) {
        if (!s.pending) return;
        check(srcnn_stream_sync(s.stream), "frame");
        const std::string fl = "FRAME" + s.params + "\n";
        if (std::fwrite(fl.data(), 1, fl.size(), out) != fl.size() || std::fwrite(s.pin_out, 1, out_bytes, out) != out_bytes)
            die(1, "write error");
        s.pending = false;
    };
    const size_t src_pitch[3] = {0, 0, 0}, dst_pitch[3] = {0, 0, 0};
    unsigned long long n = 0;
    for (;; ++n) {
        Slot& s = slots[n % 2];
        flush(s);                                         // frame n - 2 leaves before frame n takes the slot
        if (!read_line(in, line)) break;
        if (line.compare(0, 5, "FRAME") != 0) die(2, "expected FRAME, got \"%s\"", line.substr(0, 40).c_str());
        s.params = line.substr(5);
        if (std::fread(s.pin_in, 1, in_bytes, in) != in_bytes) die(2, "truncated frame");
        check(srcnn_memcpy_h2d(s.d_in, s.pin_in, in_bytes, s.stream), "upload");
        const unsigned char* const src[3] = {s.d_in, s.d_in + in_plane[0], s.d_in + in_plane[0] + in_plane[1]};
        unsigned char* const dst[3] = {s.d_out, s.d_out + out_plane[0], s.d_out + out_plane[0] + out_plane[1]};
        if (all_formats) {
            const void* const vsrc[3] = {src[0], src[1], src[2]};
            void* const vdst[3] = {dst[0], dst[1], dst[2]};
            check(srcnn_yuv_upscale_dev(&fmt, w, h, scale, filter, vsrc, src_pitch, vdst, dst_pitch, s.stream), "srcnn_yuv_upscale_dev");
        } else {
            check(srcnn_yuv420_upscale_dev(SRCNN_YUV_I420, w, h, scale, filter, src, src_pitch, dst, dst_pitch, s.stream), "srcnn_yuv420_upscale_dev");
        }
        check(srcnn_memcpy_d2h(s.pin_out, s.d_out, out_bytes, s.stream), "download");
        s.pending = true;
    }
    flush(slots[(n + 1) % 2]);                            // the last frame (n - 1); frame n - 2 left in the loop
    if (std::fflush(out) != 0) die(1, "write error");
    for (Slot& s : slots) {
        srcnn_dev_free(s.d_in);
        srcnn_dev_free(s.d_out);
        srcnn_host_free_pinned(s.pin_in);
        srcnn_host_free_pinned(s.pin_out);
        srcnn_stream_destroy(s.stream);
    }
    if (out != stdout) std::fclose(out);
    if (in != stdin) std::fclose(in);
    std::fprintf(stderr, "srcnnyuv: %llu frames, %ux%u -> %ux%u\n", n, w, h, dw, dh);
    srcnn_shutdown();
    return 0;
}
