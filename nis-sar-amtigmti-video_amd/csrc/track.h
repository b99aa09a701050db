// Internal launch interface of the GMTI tracker (track.hip) for the C ABI (api_track.hip, include/sarx_track.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sarx_track.h"

static_assert(sizeof(sarx_track_params) == 64, "sarx_track_params is 64 bytes");
static_assert(sizeof(sarx_track_header) == 64, "sarx_track_header is 64 bytes");
static_assert(sizeof(sarx_track_slot) == 96, "sarx_track_slot is 96 bytes");

namespace sarx {

// workspace: best_r[max_tracks], best_t[max_detections], free_slot[max_tracks] (int32 each, every array a multiple of 16 bytes)
inline size_t track_ws_words(int n) { return ((size_t)n + 3) & ~(size_t)3; }
inline size_t track_workspace_bytes(int max_tracks, int max_det) {
    return (2 * track_ws_words(max_tracks) + track_ws_words(max_det)) * sizeof(int32_t);
}

struct TrackArgs {
    sarx_track_params p;
    const sarx_gmti_header* slot_hdr;
    const sarx_gmti_report* rep;
    sarx_track_header* hdr;
    sarx_track_slot* slots;
    int32_t* assoc;                        // or NULL
    int32_t* best_r;                       // [max_tracks]
    int32_t* best_t;                       // [max_detections]
    int32_t* free_slot;                    // [max_tracks]
    int frame;
};
hipError_t launch_track_init(sarx_track_header* hdr, sarx_track_slot* slots, int max_tracks, hipStream_t st);
hipError_t launch_track_step(const TrackArgs& a, hipStream_t st);

}  // namespace sarx
