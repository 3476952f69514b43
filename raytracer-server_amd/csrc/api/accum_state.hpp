// The accumulator behind rt_accum_* (include/rt_ffi.h): its state, the layout of its lazily made device buffers,
// and what accum.cpp defines for the other units that work on one.
#pragma once

#include "../kernels/accum.h"
#include "api_common.hpp"

namespace rt::api {

// Progressive accumulation ----------------------------------------------------------------

// The device memory comes lazily (rt_ffi.h): the sums with the first pass, the staging area (a pass's sub, a variance
// image, an RGB8 frame) with the first call that needs one. rt_accum_add and the host forms run on a stream of their
// own that lives for the call, as rt_render's does. (The handle the ABI gives out is a void*, so the type is the
// units' own.)
struct rt_accum {
    int32_t device = 0, width = 0, height = 0;
    int64_t K = 0, N = 0;
    double* S = nullptr;
    double* Q = nullptr;
    char* stage = nullptr;
    // rendering to an error target: the per-pixel counts cnt[pix][2] = (K_p, N_p) head a buffer made by
    // the first sparse merge or selection; they are valid (and used) once a sparse pass has been merged
    char* adapt = nullptr;
    bool sparse = false;
    // seeded by rt_accum_reproject: S, Q and the per-pixel counts hold reprojected history although
    // no full-frame pass has been merged since (K = N = 0), so the next merge adds instead of storing
    bool seeded = false;
    // covered by rt_accum_fill: a seeded accumulator whose every K_p >= 2 without two full-frame
    // passes; it passes wherever K >= 1 or K >= 2 is asked for
    bool covered = false;
    // batched passes: the plan's and the expansion's buffers, made by the first call that needs them
    char* batch = nullptr;

    size_t npix() const { return (size_t)width * height; }
    size_t sub_bytes() const { return npix() * 12 * sizeof(double); }

    // The staging area: sub | var | rgb.
    double* stage_sub() const { return (double*)stage; }
    float* stage_var() const { return (float*)(stage + sub_bytes()); }
    uint8_t* stage_rgb() const { return (uint8_t*)(stage + sub_bytes() + npix() * 4 * sizeof(float)); }
    size_t stage_bytes() const { return sub_bytes() + npix() * 4 * sizeof(float) + align_up(npix() * 3, 16); }

    // The accumulator's error-target buffers: cnt | list | selection scratch | total.
    // (the scratch and the total 16-byte aligned; the scratch holds 8-byte words)
    uint32_t* cnt() const { return (uint32_t*)adapt; }
    uint32_t* adapt_list() const { return (uint32_t*)(adapt + npix() * 8); }
    size_t adapt_scratch_at() const { return align_up(npix() * 12, 16); }
    void* adapt_scratch() const { return adapt + adapt_scratch_at(); }
    size_t adapt_total_at() const { return adapt_scratch_at() + align_up(rt::select_scratch_bytes((long)npix()), 16); }
    uint32_t* adapt_total() const { return (uint32_t*)(adapt + adapt_total_at()); }
    size_t adapt_bytes() const { return adapt_total_at() + 16; }

    // The accumulator's batch buffers: want | counts | off | units | expansion scratch | words | seeds.
    // (words: hist[17] at 0, the expansion's unit total at 20; 16-byte aligned parts)
    uint8_t* batch_want() const { return (uint8_t*)batch; }
    size_t batch_counts_at() const { return align_up(npix(), 16); }
    uint8_t* batch_counts() const { return (uint8_t*)(batch + batch_counts_at()); }
    size_t batch_off_at() const { return 2 * align_up(npix(), 16); }
    uint32_t* batch_off() const { return (uint32_t*)(batch + batch_off_at()); }
    size_t batch_units_at() const { return batch_off_at() + align_up(npix() * 4, 16); }
    uint32_t* batch_units() const { return (uint32_t*)(batch + batch_units_at()); }
    size_t batch_runs_at() const { return batch_units_at() + align_up(npix() * 4, 16); }
    void* batch_runs() const { return batch + batch_runs_at(); }
    size_t batch_words_at() const { return batch_runs_at() + align_up(rt::runs_scratch_bytes((long)npix()), 16); }
    uint32_t* batch_words() const { return (uint32_t*)(batch + batch_words_at()); }
    size_t batch_seeds_at() const { return batch_words_at() + 128; }
    uint64_t* batch_seeds() const { return (uint64_t*)(batch + batch_seeds_at()); }
    size_t batch_bytes() const { return batch_seeds_at() + RT_PASSES_MAX * sizeof(uint64_t); }
};

// Makes the accumulator's device state ready for the entry point `who`, after its checks that need no device: the
// ordinal names a visible device, which is selected; the sums exist, and what the call needs of the staging area
// and of the error-target buffers.
int accum_ready(const char* who, rt_accum* a, bool stage, bool adapt);

// accum_ready plus the batch buffers.
int batch_ready(const char* who, rt_accum* a);

// Merges the pass in d_sub on `st`, waits for it and counts it.
int accum_merge(rt_accum* a, const double* d_sub, int32_t n, hipStream_t st);

// Merges the compact pass d_sub of the device list d_pixels on `st` and waits for it; the first sparse merge fills the
// per-pixel counts with the frame's (K, N). The merge launch is the varying part: one pass per pixel, or with d_counts
// and d_off (device, n_pixels entries) the run merge of a batched pass, d_counts[e] passes of pixel e from unit d_off[e] on.
int accum_merge_list(rt_accum* a, const uint32_t* d_pixels, int64_t n_pixels, const double* d_sub, int32_t n,
                     hipStream_t st, const uint8_t* d_counts = nullptr, const uint32_t* d_off = nullptr);

// Enqueues the resolve on `st`: sub (or, when only the RGB8 is wanted, the staging sub), var, rgb.
hipError_t accum_resolve_enqueue(rt_accum* a, double* d_sub, float* d_var, uint8_t* d_rgb, hipStream_t st);

int check_accum_add(const rt_accum* a, const rt_scene* scene, const rt_render_params* p);
int check_accum_sub(const char* who, const rt_accum* a, const void* sub, int32_t n);
int check_accum_resolve(const char* who, const rt_accum* a, const void* var);

// host_list: the list is on the host and checked (strictly ascending ids below width * height).
int check_sparse(const char* who, const rt_accum* a, const void* pixels, int64_t n_pixels, bool host_list);

}  // namespace rt::api
