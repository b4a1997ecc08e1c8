// What the record conditioners (bds_blank.hip, bds_notch.hip) share on the host: the checks of an entry's pointers, the choice
// of a kernel's sample layout, and the loop that takes a window through the device piece by piece on the context's two streams.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "bds_internal.h"
#include "bds_record_window.h"

namespace bds {

// ---- entry checks -----------------------------------------------------------------------------------------------------------------
// What every entry checks first: the format, then the options and the report against the sample count (the conditioner's own
// format_of and check_args).  fmt (>= 0) or BDS_ERR_*.
template <class Opts, class Out>
int check_entry(bds_ctx *ctx, const char *who, int (*format_of)(const bds_settings *, const char **),
                int (*check_args)(int, int64_t, int64_t, const Opts *, const Out *, int64_t *, char *, size_t), const bds_settings *s, int64_t n_bytes,
                int64_t n, const Opts *o, const Out *rep, int64_t *n_samples) {
    const char *why;
    const int fmt = format_of(s, &why);
    if (fmt < 0) return fail(ctx, fmt, "%s: %s", who, why);
    char msg[256];
    if (int rc = check_args(fmt, n_bytes, n, o, rep, n_samples, msg, sizeof msg)) return fail(ctx, rc, "%s: %s", who, msg);
    return fmt;
}

// The two buffers of an entry on host memory; `out` counts only when the call writes.  The context is looked at last.
inline int check_host_pair(bds_ctx *ctx, const char *who, const void *in, const void *out, size_t n_bytes, bool writes) {
    if (n_bytes && (!in || (writes && !out))) return fail(ctx, BDS_ERR_ARG, "%s: in or out is NULL", who);
    if (writes && partial_overlap(in, out, n_bytes)) return fail(ctx, BDS_ERR_ARG, "%s: in and out overlap in part (they must be the same buffer or disjoint)", who);
    if (!ctx) return fail(ctx, BDS_ERR_ARG, "%s: ctx is NULL", who);
    return BDS_OK;
}

// The two buffers of a _dev entry: aligned to the record's elements, the same or disjoint, each inside one device allocation.
inline int check_device_pair(bds_ctx *ctx, const char *who, int fmt, const void *d_in, const void *d_out, size_t n_bytes, bool writes) {
    const int el = probe::elem_bytes(fmt);
    if (reinterpret_cast<uintptr_t>(d_in) % (uintptr_t)el || (writes && reinterpret_cast<uintptr_t>(d_out) % (uintptr_t)el))
        return fail(ctx, BDS_ERR_ARG, "%s: d_in or d_out is not aligned to the %d-byte samples of the record", who, el);
    if (writes && partial_overlap(d_in, d_out, n_bytes))
        return fail(ctx, BDS_ERR_ARG, "%s: d_in and d_out overlap in part (they must be the same buffer or disjoint)", who);
    if (int rc = check_device_span(ctx, who, "d_in", d_in, n_bytes)) return rc;
    return writes ? check_device_span(ctx, who, "d_out", d_out, n_bytes) : BDS_OK;
}

// f(SB, E) with the bytes of a sample and of one of its elements as compile-time constants: f's body names a kernel template
// by decltype(sb)::value, decltype(e)::value.
template <class F>
void with_sample_layout(int fmt, F f) {
    using std::integral_constant;
    switch (fmt) {
    case probe::kS8: f(integral_constant<int, 1>{}, integral_constant<int, 1>{}); break;
    case probe::kS8C: f(integral_constant<int, 2>{}, integral_constant<int, 1>{}); break;
    case probe::kS16: f(integral_constant<int, 2>{}, integral_constant<int, 2>{}); break;
    default: f(integral_constant<int, 4>{}, integral_constant<int, 2>{}); break;
    }
}

// ---- the piece loop ---------------------------------------------------------------------------------------------------------------
// A window goes through the device in n_pieces pieces on the context's two streams.  Piece k uses slot k & 1: that stream, a
// device buffer and a pinned buffer of buf_bytes each, a pinned block of result_bytes and an event, all owned by the loop.
//   setup()                        -> hipError_t   the conditioner's own device memory and tables; not called for an empty window
//   span_of(k)                     -> Span         the bytes of the window that piece k loads
//   read(first_byte, n_bytes, dst) -> BDS_*        fills the pinned buffer on this thread
//   work(k, slot)                  -> hipError_t   enqueues on slot.stream all that lies between the upload of slot.d_buf and the
//                                                  event: the kernels, the download of the bytes wanted back into slot.h_buf and of
//                                                  the small results into slot.h_res
//   take(k, slot)                  -> BDS_*        on this thread once the event has come: hands the bytes on, adds the sums
// What callers rely on, and nothing else in the tree says:
//   * The order on this thread is read(k), enqueue k, take(k - 1).  bds_blank in place on host memory needs piece k read before
//     piece k - 1 is written back.
//   * Slot k & 1 is free for piece k because take(k - 2) has returned before read(k) begins.
//   * Per piece there is one upload of span_of(k).bytes; every other copy is work's.
//   * n_pieces == 0 allocates nothing, calls nothing and launches nothing.
//   * Both streams are synchronised before anything is released, on every path; a callback's BDS_* code comes back as it is
//     (its message is set), a HIP error as BDS_ERR_NOMEM / BDS_ERR_HIP (hip_fail).
namespace pipe {

struct Slot {
    hipStream_t stream = nullptr;
    uint8_t *d_buf = nullptr, *h_buf = nullptr, *h_res = nullptr;
    hipEvent_t done = nullptr;
};
struct Span {
    int64_t first_byte;
    size_t bytes;
};
// read and write of a window that lies in host memory
inline auto from_memory(const void *src) {
    return [src](int64_t at, size_t n, uint8_t *to) { return std::memcpy(to, static_cast<const uint8_t *>(src) + at, n), (int)BDS_OK; };
}
inline auto to_memory(void *dst) {
    return [dst](int64_t at, size_t n, const uint8_t *from) { return std::memcpy(static_cast<uint8_t *>(dst) + at, from, n), (int)BDS_OK; };
}

template <class Setup, class SpanOf, class Read, class Work, class Take>
int run(bds_ctx *ctx, const char *who, int64_t n_pieces, size_t buf_bytes, size_t result_bytes, Setup setup, SpanOf span_of, Read read, Work work, Take take) {
    int rc = BDS_OK;
    hipError_t e = hipSetDevice(ctx->device);
    DevScope scope;
    Slot slot[2];
    slot[0].stream = (hipStream_t)ctx->stream, slot[1].stream = (hipStream_t)ctx->stream2;
    for (int i = 0; i < 2 && e == hipSuccess && n_pieces; ++i) {
        e = scope.alloc(&slot[i].d_buf, buf_bytes);
        if (e == hipSuccess) e = scope.pinned(&slot[i].h_buf, buf_bytes);
        if (e == hipSuccess) e = scope.pinned(&slot[i].h_res, result_bytes);
        if (e == hipSuccess) e = scope.event(&slot[i].done);
    }
    if (e == hipSuccess && n_pieces) e = setup();
    auto finish = [&](int64_t k) {  // wait for piece k, then the host's part of it
        Slot &s = slot[k & 1];
        e = hipEventSynchronize(s.done);
        if (e == hipSuccess) rc = take(k, s);
    };
    for (int64_t k = 0; k < n_pieces && !rc && e == hipSuccess; ++k) {
        Slot &s = slot[k & 1];
        const Span sp = span_of(k);
        rc = read(sp.first_byte, sp.bytes, s.h_buf);  // (piece k - 2, the last user of these buffers, is finished)
        if (rc) break;
        e = hipMemcpyAsync(s.d_buf, s.h_buf, sp.bytes, hipMemcpyHostToDevice, s.stream);
        if (e == hipSuccess) e = work(k, s);
        if (e == hipSuccess) e = hipEventRecord(s.done, s.stream);
        if (e == hipSuccess && k >= 1) finish(k - 1);
    }
    if (!rc && e == hipSuccess && n_pieces) finish(n_pieces - 1);
    (void)hipStreamSynchronize(slot[0].stream);  // nothing of this call may still run when its buffers go
    (void)hipStreamSynchronize(slot[1].stream);
    if (rc) return rc;
    return e == hipSuccess ? BDS_OK : hip_fail(ctx, who, e);
}

}  // namespace pipe
}  // namespace bds
