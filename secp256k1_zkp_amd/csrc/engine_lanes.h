// engine_lanes.h -- what a family does around its kernels, written once (host code only):
//   lanes_run               the `_dev` form of a one-item-per-lane family: device, lock, stream, tables, zeroed outputs, events, the sub-range loop
//   stage_open / _close     the host-buffer form of every family: each buffer named once, carved from the workspace (beside the device part's
//                           own workspace, where it has one), uploaded, downloaded.  The stager owns the ordering of its uploads: stage_open
//                           first makes e->stream wait for the engine's last work when that was queued on another stream (stream_guard),
//                           so a host form opens no guard of its own in front of it.
//                           (Not staged here: the rangeproof verify host path, rp_host_submit / rp_host_wait -- pinned staging sets, a copy
//                           stream, two batches in flight and a lifetime that outlasts the call.)
//   der_window              the bytes and rebased offsets of a DER-packed signature array
// An entry point keeps its own prologue (who, null engine, n == 0, ARG_CHECK, formats) and hands the rest to these.
#pragma once
#include "engine_internal.h"
#include "ecdsa.h"        // ECDSA_SIG_DER

// ------------------------------------------------------------------------------------------------------------
// the lane-launch scaffold
// ------------------------------------------------------------------------------------------------------------
// A parking area lies behind the per-lane tables in the engine's table buffer: word k of lane i of a launch of L lanes at
// park[k * L + i], so a wavefront's store or load of one word is 256 contiguous bytes.
static inline size_t park_lanes(size_t lanes, size_t words) { return (lanes * words + S2K_PTAB_WORDS - 1) / S2K_PTAB_WORDS; }      // the area, counted in table slices

struct lanes_need { bool gtab; bool ptab; size_t park_words; };   // park_words: words per lane parked behind the tables, else 0
struct zero_span { void* p; size_t bytes; };

// launch(i0, m, grid, st, park) holds the hipLaunchKernelGGL call(s) of the sub-range [i0, i0 + m): it runs under the engine's lock and
// reads e->gtab / e->ptab there.  `zero`: outputs that a batch which does not complete must not leave looking valid.
template <class Launch>
static int lanes_run(s2k_engine* e, void* stream, size_t n, lanes_need need, std::initializer_list<zero_span> zero, Launch launch) {
    HIPCHK(hipSetDevice(e->device));
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    hipStream_t st = stream ? (hipStream_t)stream : e->stream;
    stream_guard sg(e, st);
    u32* park = nullptr;
    if (need.ptab) {
        const size_t lanes = ((std::min(n, e->max_lanes) + 255) / 256) * 256;
        if (!engine_ptab(e, lanes + (need.park_words ? park_lanes(lanes, need.park_words) : 0))) return 0;
        if (need.park_words) park = e->ptab + lanes * S2K_PTAB_WORDS;
    }
    if (need.gtab) ENGINE_GTAB(e, st);
    for (const zero_span& z : zero) HIPCHK(hipMemsetAsync(z.p, 0, z.bytes, st));
    HIPCHK(hipEventRecord(e->ev[0], st)); HIPCHK(hipEventRecord(e->ev[2], st));
    for (size_t i0 = 0; i0 < n; i0 += e->max_lanes) {
        const size_t m = std::min(n - i0, e->max_lanes);                  // (m <= lanes: every launch's park stride fits the area)
        launch(i0, m, dim3((unsigned)((m + 255) / 256)), st, park);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->ev[3], st)); HIPCHK(hipEventRecord(e->ev[1], st));
    return 1;
}

// ------------------------------------------------------------------------------------------------------------
// the host stager
// ------------------------------------------------------------------------------------------------------------
// One buffer of a host-buffer form.  in: uploaded when non-null and bytes != 0; out: downloaded at the end; neither: scratch, or an
// optional input the caller left out (it keeps its slot in the carve, and opt() hands nullptr on to the `_dev` form).  pad: bytes behind
// the buffer that a kernel's read-ahead may touch.  dev: where stage_open put it.
struct stage_buf {
    const void* in; void* out; size_t bytes, pad; unsigned char* dev;
    template <class T = unsigned char> T* at() const { return (T*)dev; }
    template <class T = unsigned char> T* opt() const { return in ? (T*)dev : nullptr; }
};
// where the last buffer ends when the first one starts at a 256-byte boundary
template <size_t N>
static size_t stage_end(const stage_buf (&b)[N]) {
    size_t t = 0;
    for (const stage_buf& s : b) t = ((t + 255) & ~size_t(255)) + s.bytes + s.pad;
    return t;
}
// the staged size (the ws_need rule over bytes + pad): with the buffers at offset 0, where a carve behind them starts
template <size_t N>
static size_t stage_bytes(const stage_buf (&b)[N]) { return (stage_end(b) + 255) & ~size_t(255); }
// sizes the workspace, carves the buffers in order from offset lo and queues the uploads on e->stream.  A form whose device part has a
// workspace of its own says where it lies: in front of the buffers ([0, lo): the carves that start at 0 again, such as a locating call's)
// or behind them (extra bytes from stage_bytes(b) on; lo = 0).  The uploads overwrite a workspace that the call before this one may still
// be reading on a caller's stream: they are queued under a stream_guard, which leaves last_stream == e->stream, so the guard that the
// device part opens next (the `_dev` form's own, or the host form's behind stage_open) finds nothing to wait for.
template <size_t N>
static int stage_open(s2k_engine* e, stage_buf (&b)[N], size_t lo = 0, size_t extra = 0) {
    if (!engine_workspace(e, lo + stage_end(b) + 256 + extra)) return 0;      // (sized once: growing the workspace moves it)
    ws_carver w{e->ws, lo};
    for (stage_buf& s : b) s.dev = w.take<unsigned char>(s.bytes + s.pad);
    stream_guard sg(e, e->stream);
    for (const stage_buf& s : b) if (s.in && s.bytes) HIPCHK(hipMemcpyAsync(s.dev, s.in, s.bytes, hipMemcpyHostToDevice, e->stream));
    return 1;
}
// ok: what the `_dev` form returned.  Either way nothing of the call is in flight when this returns.
template <size_t N>
static int stage_close(s2k_engine* e, stage_buf (&b)[N], int ok) {
    if (!ok) { (void)hipStreamSynchronize(e->stream); return 0; }
    for (const stage_buf& s : b) if (s.out) HIPCHK(hipMemcpyAsync(s.out, s.dev, s.bytes, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return 1;
}

// DER-packed signatures: the items' bytes [sig_off[0], sig_off[n]) go to HBM as they are, with offsets relative to their start.
// Other formats: 64 bytes per item and no offsets.
struct der_span { const unsigned char* lo; size_t bytes; std::vector<uint64_t> rel; };
static inline int der_window(const char* who, der_span& w, const unsigned char* sigs, const uint64_t* sig_off, int sig_format, size_t n) {
    w.lo = sigs; w.bytes = 64 * n;
    if (sig_format != ECDSA_SIG_DER) return 1;
    for (size_t i = 0; i < n; i++) if (sig_off[i + 1] < sig_off[i]) return s2k_fail_arg(who, "sig_off must not decrease");
    w.lo = sigs + sig_off[0]; w.bytes = (size_t)(sig_off[n] - sig_off[0]);
    w.rel.resize(n + 1);
    for (size_t i = 0; i <= n; i++) w.rel[i] = sig_off[i] - sig_off[0];
    return 1;
}
