// abi.h -- what every file that defines C entry points (include/surfel_raster.h) needs: the refusal, the HIP-error macro, the per-device
// and per-thread services api.hip keeps, and the two argument checks that more than two ops state word for word.  An op's own entry points
// sit at the end of its .hip file, under "---- C-ABI ----"; a check that is specific to one op stays written out there.  (The rasteriser's
// entry points, in api.hip, check (frame, g) and their state buffers in one place of their own: api.hip Call.)
// No device code.  Defined in api.hip: fail, stream_device, rank_mode, pinned_words.
#pragma once
#include "launch.h"

namespace sr {

// stores the formatted text for sr_last_error() (per calling thread) and returns `code`
int fail(int code, const char* fmt, ...);

#define SR_HIP(expr)                                                                                             \
    do {                                                                                                         \
        hipError_t _e = (expr);                                                                                  \
        if (_e != hipSuccess) return sr::fail(SR_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                                              __FILE__, __LINE__);                                               \
    } while (0)

// the device a stream belongs to; the null stream -> the current device
int stream_device(hipStream_t s, int* dev);
// how the sort / partition kernels rank items inside a wave on the stream's device (self-checked once per device, then cached)
int rank_mode(hipStream_t s, bool force_ballot, RankMode* mode);
// the calling thread's 64-B pinned host block, or nullptr (api.hip states which words are whose)
uint32_t* pinned_words();

// A caller's workspace: not NULL, then at least `need` bytes.  `who`: the "name: " in front of the texts (the auxiliary losses and the sky
// model name their entry point); `short_code`: what a short workspace returns (sr_mesh_count / sr_mesh_emit: SR_ERR_INVALID_ARGUMENT).
inline int check_workspace_size(const void* workspace, size_t bytes, size_t need, const char* who = nullptr, int short_code = SR_ERR_BUFFER_TOO_SMALL) {
    const char* sep = who ? ": " : "";
    if (!who) who = "";
    if (!workspace) return fail(SR_ERR_INVALID_ARGUMENT, "%s%sworkspace is NULL", who, sep);
    if (bytes < need) return fail(short_code, "%s%sworkspace %zu < %zu", who, sep, bytes, need);
    return SR_OK;
}
// ... and, for the ops whose kernels read it in 16-B words, 16-B aligned
inline int check_workspace(const void* workspace, size_t bytes, size_t need, int short_code = SR_ERR_BUFFER_TOO_SMALL) {
    if (int rc = check_workspace_size(workspace, bytes, need, nullptr, short_code)) return rc;
    if ((uintptr_t)workspace & 15u) return fail(SR_ERR_INVALID_ARGUMENT, "workspace is not 16-B aligned");
    return SR_OK;
}

// An array that is float32 or float64 by a flag: the flag is 0 or 1, then the address (NULL passes) is aligned to the element size.
inline int check_f32_or_f64(const char* name, const void* p, int is_f64) {
    if (is_f64 != 0 && is_f64 != 1) return fail(SR_ERR_INVALID_ARGUMENT, "%s_f64 = %d: 0 (float32) or 1 (float64)", name, is_f64);
    if ((uintptr_t)p & (is_f64 ? 7u : 3u)) return fail(SR_ERR_INVALID_ARGUMENT, "%s is not aligned to its element size", name);
    return SR_OK;
}

}  // namespace sr
