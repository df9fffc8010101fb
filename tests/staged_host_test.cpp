// Host-only check of eftpipe_amd/csrc/eftb_staged.hpp (tests/test_staged_host.py compiles and runs it under the address and
// undefined-behaviour sanitizers).  Every expected value below was worked out by hand from the layout in main().
#include <cstdio>

#include "eftb_staged.hpp"

using namespace eftb;

static int failures = 0;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

static void check_seg(const UploadSegs& sg, int i, int step, size_t src, size_t dst, unsigned n, unsigned first, int line) {
    const UploadSeg& g = sg.s[i];
    if (g.step != step || g.src_off != src || g.dst_off != dst || g.n != n || g.first != first) {
        std::printf("line %d: segment %d is (step %d, src %zu, dst %zu, n %u, first %u), expected (%d, %zu, %zu, %u, %u)\n", line, i, g.step, g.src_off,
                    g.dst_off, g.n, g.first, step, src, dst, n, first);
        ++failures;
    }
}
#define SEG(sg, i, step, src, dst, n, first) check_seg(sg, i, step, src, dst, n, first, __LINE__)

static void check_span(const OutSpan& s, int step, int row, int rows, bool own, int line) {
    if (s.step != step || s.row != row || s.rows != rows || s.own != own) {
        std::printf("line %d: span is (step %d, row %d, rows %d, own %d), expected (%d, %d, %d, %d)\n", line, s.step, s.row, s.rows, (int)s.own, step, row,
                    rows, (int)own);
        ++failures;
    }
}
#define SPAN(s, step, row, rows, own) check_span(s, step, row, rows, own, __LINE__)

int main() {
    // 100 P_lin samples, f, DA, H, 24 bias entries and 2 x 24 likelihood rows per cosmology; a step brings 4 cosmologies at most, a set
    // holds 32: a staging block is PIN 0, F 400, DA 404, H 408, BIAS 412, GROWS 508; a set's block PIN 0, F 3200, DA 3232, H 3264, BIAS 3296,
    // GROWS 4064
    UploadLayout lay{};
    const size_t width[6] = {100, 1, 1, 1, 24, 48}, slot_off[6] = {0, 400, 404, 408, 412, 508}, stage_off[6] = {0, 3200, 3232, 3264, 3296, 4064};
    for (int a = 0; a < 6; ++a) {
        lay.width[a] = width[a];
        lay.slot_off[a] = slot_off[a];
        lay.stage_off[a] = stage_off[a];
        lay.present[a] = true;
    }

    {  // one step of 3 cosmologies, with rows
        const int B[1] = {3};
        const UploadSegs sg = upload_segments(lay, B, 1, 0, 6);
        CHECK(sg.n == 6);
        SEG(sg, 0, 0, 0, 0, 300, 0);        // 300 -> 320 lanes
        SEG(sg, 1, 0, 400, 3200, 3, 320);
        SEG(sg, 2, 0, 404, 3232, 3, 384);
        SEG(sg, 3, 0, 408, 3264, 3, 448);
        SEG(sg, 4, 0, 412, 3296, 72, 512);  // 72 -> 128 lanes
        SEG(sg, 5, 0, 508, 4064, 144, 640); // 144 -> 192 lanes
        CHECK(sg.total == 832);
    }
    {  // MAX_COALESCE steps of 4 with rows: exactly the capacity; a step takes 448 + 3 * 64 + 128 + 192 = 960 lanes
        const int B[8] = {4, 4, 4, 4, 4, 4, 4, 4};
        static_assert(MAX_COALESCE == 8 && MAX_UPLOAD_SEGS == 48, "the case below is written for 8 steps x 6 arrays");
        const UploadSegs sg = upload_segments(lay, B, 8, 0, 6);
        CHECK(sg.n == 48);
        for (int i = 0; i < sg.n; ++i) CHECK(sg.s[i].first % 64 == 0);
        SEG(sg, 0, 0, 0, 0, 400, 0);
        SEG(sg, 5, 0, 508, 4064, 192, 768);
        SEG(sg, 6, 1, 0, 400, 400, 960);
        SEG(sg, 7, 1, 400, 3204, 4, 1408);
        SEG(sg, 10, 1, 412, 3392, 96, 1600);
        SEG(sg, 42, 7, 0, 2800, 400, 6720);
        SEG(sg, 47, 7, 508, 5408, 192, 7488);
        CHECK(sg.total == 7680);
    }
    {  // two steps (2 and 3 cosmologies) without rows: the GROWS array does not travel
        UploadLayout norows = lay;
        norows.present[5] = false;
        const int B[2] = {2, 3};
        const UploadSegs sg = upload_segments(norows, B, 2, 0, 6);
        CHECK(sg.n == 10);
        SEG(sg, 0, 0, 0, 0, 200, 0);
        SEG(sg, 1, 0, 400, 3200, 2, 256);
        SEG(sg, 2, 0, 404, 3232, 2, 320);
        SEG(sg, 3, 0, 408, 3264, 2, 384);
        SEG(sg, 4, 0, 412, 3296, 48, 448);
        SEG(sg, 5, 1, 0, 200, 300, 512);
        SEG(sg, 6, 1, 400, 3202, 3, 832);
        SEG(sg, 7, 1, 404, 3234, 3, 896);
        SEG(sg, 8, 1, 408, 3266, 3, 960);
        SEG(sg, 9, 1, 412, 3344, 72, 1024);
        CHECK(sg.total == 1152);
    }
    {  // latency mode: the small arrays [1, 6) first, then P_lin [0, 1); one step of 3, no rows
        UploadLayout norows = lay;
        norows.present[5] = false;
        const int B[1] = {3};
        const UploadSegs small = upload_segments(norows, B, 1, 1, 6);
        CHECK(small.n == 4);
        SEG(small, 0, 0, 400, 3200, 3, 0);
        SEG(small, 1, 0, 404, 3232, 3, 64);
        SEG(small, 2, 0, 408, 3264, 3, 128);
        SEG(small, 3, 0, 412, 3296, 72, 192);
        CHECK(small.total == 320);
        const UploadSegs pin = upload_segments(norows, B, 1, 0, 1);
        CHECK(pin.n == 1);
        SEG(pin, 0, 0, 0, 0, 300, 0);
        CHECK(pin.total == 320);
    }

    // span merging: three steps of 2, 3 and 1 cosmologies, 10 doubles per cosmology
    static double buf[100];
    const int B[3] = {2, 3, 1};
    OutSpan sp[3];
    {  // no destinations: one transfer to the set's block
        const double* out[3] = {nullptr, nullptr, nullptr};
        CHECK(merge_out_spans(out, B, 3, 10, sp) == 1);
        SPAN(sp[0], 0, 0, 6, false);
    }
    {  // destinations that follow each other in memory: one transfer
        const double* out[3] = {buf, buf + 20, buf + 50};
        CHECK(merge_out_spans(out, B, 3, 10, sp) == 1);
        SPAN(sp[0], 0, 0, 6, true);
    }
    {  // a gap behind the first destination; the other two are contiguous
        const double* out[3] = {buf, buf + 30, buf + 60};
        CHECK(merge_out_spans(out, B, 3, 10, sp) == 2);
        SPAN(sp[0], 0, 0, 2, true);
        SPAN(sp[1], 1, 2, 4, true);
    }
    {  // a step without a destination between two that have one (which would be contiguous without it)
        const double* out[3] = {buf, nullptr, buf + 20};
        CHECK(merge_out_spans(out, B, 3, 10, sp) == 3);
        SPAN(sp[0], 0, 0, 2, true);
        SPAN(sp[1], 1, 2, 3, false);
        SPAN(sp[2], 2, 5, 1, true);
    }
    {  // a single step, without and with a destination
        const double* none[1] = {nullptr};
        CHECK(merge_out_spans(none, B, 1, 10, sp) == 1);
        SPAN(sp[0], 0, 0, 2, false);
        const double* own[1] = {buf + 7};
        CHECK(merge_out_spans(own, B, 1, 10, sp) == 1);
        SPAN(sp[0], 0, 0, 2, true);
    }
    if (failures) std::printf("%d check(s) failed\n", failures);
    else std::printf("staged_host_test: all checks passed\n");
    return failures ? 1 : 0;
}
