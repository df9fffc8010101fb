// eftb_staged.hpp -- the two pure pieces of a staged launch (eftbird.hip: launch_upload, copy_out): which runs of doubles the upload kernel
// moves, and which transfers carry P_l out.  Offsets and counts only: no HIP include, no engine, so a host compiler alone builds it
// (tests/test_staged_host.py runs tests/staged_host_test.cpp under the address and undefined-behaviour sanitizers).
#pragma once

#include <cstddef>

namespace eftb {

constexpr int MAX_COALESCE = 8;   // steps one launch carries at most (staged_setup's clamp of coalesce_max, sub_main's group)
constexpr int STAGED_ARRAYS = 6;  // arrays of a staging block, in kStagedIn's order: PIN, F, DA, H, BIAS, GROWS
constexpr int MAX_UPLOAD_SEGS = MAX_COALESCE * STAGED_ARRAYS;

// layout of the staged arrays: doubles per cosmology, where the array starts in a step's staging block and in a set's device block, and
// whether it travels at all (the configuration has it; the likelihood rows: the steps brought some)
struct UploadLayout {
    size_t width[STAGED_ARRAYS], slot_off[STAGED_ARRAYS], stage_off[STAGED_ARRAYS];
    bool present[STAGED_ARRAYS];
};

// one run of doubles: from src_off of step `step`'s staging block to dst_off of the set's device block.  first: index of the run's first
// element in the launch's flat numbering, a multiple of 64 (stage_gather_kernel picks a lane's run by it: the choice is wave-uniform)
struct UploadSeg { int step; size_t src_off, dst_off; unsigned n, first; };
struct UploadSegs { UploadSeg s[MAX_UPLOAD_SEGS]; int n; unsigned total; };  // total: lanes of the launch

// arrays [lo, hi) of every step of a group (B[j] cosmologies each): the steps' rows follow each other in the device block
inline UploadSegs upload_segments(const UploadLayout& lay, const int* B, int nsteps, int lo, int hi) {
    UploadSegs sg{};
    int row = 0;
    for (int j = 0; j < nsteps; ++j) {
        for (int a = lo; a < hi; ++a) {
            if (!lay.present[a]) continue;
            UploadSeg& g = sg.s[sg.n++];
            g.step = j;
            g.src_off = lay.slot_off[a];
            g.dst_off = lay.stage_off[a] + (size_t)row * lay.width[a];
            g.n = (unsigned)((size_t)B[j] * lay.width[a]);
            g.first = sg.total;
            sg.total += (g.n + 63u) & ~63u;
        }
        row += B[j];
    }
    return sg;
}

// one transfer of P_l: `rows` cosmologies from row `row` of the launch, to step `step`'s own destination (own) or to the same rows of the
// set's host block
struct OutSpan { int step, row, rows; bool own; };

// Steps next to each other without a destination of their own travel as one transfer; so do steps whose destinations follow each other in
// memory (the slices of one results array); everything else is a transfer of its own.  out[j]: step j's destination or null; per: doubles
// per cosmology.  Returns the number of spans (at most nsteps).
inline int merge_out_spans(const double* const* out, const int* B, int nsteps, size_t per, OutSpan* spans) {
    int ns = 0, row = 0;
    for (int j = 0; j < nsteps;) {
        int j1 = j + 1, rows = B[j];
        if (!out[j])
            for (; j1 < nsteps && !out[j1]; ++j1) rows += B[j1];
        else
            for (; j1 < nsteps && out[j1] == out[j] + (size_t)rows * per; ++j1) rows += B[j1];
        spans[ns++] = OutSpan{j, row, rows, out[j] != nullptr};
        row += rows;
        j = j1;
    }
    return ns;
}

}  // namespace eftb
