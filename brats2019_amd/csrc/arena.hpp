// arena.hpp -- the one workspace allocator of the library: the network executor (engine.hip) and the op-level entry points (op_abi.hip) carve
// with it, and every *_workspace_bytes query of theirs is the same walk over a DRY arena -- the size is whatever the real walk takes, call for call.
#pragma once
#include "ru_common.h"

namespace ru {

// Bump allocator over the caller's workspace.  Tensors grow from the bottom (`off`); an inference forward REWINDS to a mark when a
// block's temporaries are dead (everything runs on one stream, so a later kernel may overwrite them), `peak` is the high-water mark.
// Small per-layer arrays that must outlive those rewinds (GroupNorm mean / rstd / scale / shift, read by ru_unet_gn_stats and by the
// backward) are taken from the TOP of the workspace (`keep`).  A dry walk mirrors the real one call for call.
struct Arena {
    char* base = nullptr;
    size_t cap = 0, off = 0, peak = 0, keep = 0;
    bool dry = true, failed = false;
    float* alloc(size_t nfloats) {
        const size_t bytes = align_up(nfloats * sizeof(float), 256);
        const size_t o = off;
        off += bytes;
        if (off > peak) peak = off;
        if (dry) return nullptr;
        if (off + keep > (cap & ~(size_t)255)) { failed = true; return nullptr; }
        return reinterpret_cast<float*>(base + o);
    }
    float* alloc_keep(size_t nfloats) {
        keep += align_up(nfloats * sizeof(float), 256);
        if (dry) return nullptr;
        const size_t top = cap & ~(size_t)255;           // (a caller may pass any size: the top region stays 256-byte aligned)
        if (off + keep > top) { failed = true; return nullptr; }
        return reinterpret_cast<float*>(base + top - keep);
    }
    void rewind(size_t mark) { off = mark; }
    size_t need() const { return peak + keep; }
};

}  // namespace ru

// Every launch and pack call of a walk goes through this, with the walk's arena in scope as `A`: a dry arena skips the call; an arena that has
// failed refuses on the host, before anything is enqueued that would read a pointer the arena did not hand out; otherwise the call runs and
// its error is the walk's.
#define RU_ARENA_RUN(call)                \
    do {                                  \
        if (!A.dry) {                     \
            if (A.failed) { ru::set_error("workspace too small"); return RU_ENOMEM; } \
            const int rc__ = (call);      \
            if (rc__ != RU_OK) return rc__; \
        }                                 \
    } while (0)
