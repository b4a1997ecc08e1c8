// The IF record as tracking (bds_track.hip) and the correlation function (bds_corrfn.hip) read it: one class, three places a
// record can lie in, one load().
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <string>

#include "bds_internal.h"

namespace bds {

// Source of the IF record: load() copies bytes [off, off + n) of it into device memory at dst, ordered on `stream`.
//   file           read through a pinned staging buffer of at most `stage_cap` bytes, piece by piece with a synchronise per piece
//                  (the staging buffer is filled again next); the source owns the FILE* and the buffer
//   host memory    one host-to-device hipMemcpyAsync
//   device memory  one device-to-device hipMemcpyAsync; the caller has checked the range (check_device_span)
//   none           a fed session: its caller appends the samples itself, a load is an error
// A failed load has set the context's message (fail()).
// ONE thread calls load() at a time -- there is no lock.  Streamed tracking loads from its loader thread between
// SpanStream::start_load() and join(), and the main thread loads only after join().
class RecordSource {
public:
    RecordSource() = default;
    RecordSource(const RecordSource &) = delete;
    RecordSource &operator=(const RecordSource &) = delete;
    ~RecordSource() {
        if (pin_) (void)hipHostFree(pin_);
        if (file_) fclose(file_);
    }

    int open_file(bds_ctx *ctx, const char *path, size_t stage_cap) {
        ctx_ = ctx, kind_ = kFile, what_ = path;
        file_ = fopen(path, "rb");
        if (!file_) return fail(ctx, BDS_ERR_IO, "Unable to read file %s", path);  // postProcessing.m:152-154
        fseeko(file_, 0, SEEK_END);
        const long long sz = ftello(file_);
        if (sz <= 0) return fail(ctx, BDS_ERR_IO, "file %s is empty", path);
        size_ = (size_t)sz;
        pin_bytes_ = std::min(stage_cap, size_);
        BDS_HIP(ctx, hipSetDevice(ctx->device));
        if (hipHostMalloc(&pin_, pin_bytes_, 0) != hipSuccess) {
            (void)hipGetLastError();
            pin_ = nullptr;
            return fail(ctx, BDS_ERR_NOMEM, "pinned staging buffer");
        }
        return BDS_OK;
    }
    void set_host(bds_ctx *ctx, const int8_t *bytes, size_t n) { ctx_ = ctx, kind_ = kHost, mem_ = bytes, size_ = n, what_ = "a record in memory"; }
    void set_device(bds_ctx *ctx, const void *d_bytes, size_t n) {
        ctx_ = ctx, kind_ = kDevice, mem_ = (const int8_t *)d_bytes, size_ = n, what_ = "a record in device memory";
    }
    void set_none(bds_ctx *ctx) { ctx_ = ctx, kind_ = kNone, what_ = "a fed record"; }

    size_t size() const { return size_; }             // bytes of the record
    const char *what() const { return what_.c_str(); }  // for messages: the file's path, or which memory

    int load(size_t off, size_t n, int8_t *dst, hipStream_t stream) const {
        switch (kind_) {
        case kHost:
        case kDevice:
            BDS_HIP(ctx_, hipMemcpyAsync(dst, mem_ + off, n, kind_ == kHost ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, stream));
            return BDS_OK;
        case kFile:
            if (fseeko(file_, (off_t)off, SEEK_SET)) return fail(ctx_, BDS_ERR_IO, "seek in %s failed", what());
            for (size_t done = 0; done < n;) {
                const size_t m = std::min(pin_bytes_, n - done);
                if (fread(pin_, 1, m, file_) != m) return fail(ctx_, BDS_ERR_IO, "short read on %s", what());
                hipError_t e = hipMemcpyAsync(dst + done, pin_, m, hipMemcpyHostToDevice, stream);
                if (e == hipSuccess) e = hipStreamSynchronize(stream);  // the staging buffer is filled again next
                if (e != hipSuccess) return fail(ctx_, BDS_ERR_HIP, "H2D copy: %s", hipGetErrorString(e));
                done += m;
            }
            return BDS_OK;
        default:
            return fail(ctx_, BDS_ERR_ARG, "a feed session has no record to load from");
        }
    }

private:
    enum Kind { kNone, kFile, kHost, kDevice };
    bds_ctx *ctx_ = nullptr;
    Kind kind_ = kNone;
    std::string what_ = "a fed record";
    size_t size_ = 0;
    const int8_t *mem_ = nullptr;  // kHost / kDevice
    FILE *file_ = nullptr;         // kFile
    void *pin_ = nullptr;
    size_t pin_bytes_ = 0;
};

}  // namespace bds
