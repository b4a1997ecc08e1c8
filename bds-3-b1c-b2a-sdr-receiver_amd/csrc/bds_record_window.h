// The window of a record file as bds_blank_file, bds_notch_file and bds_probe_data_file take it: the samples [skip, skip + n) of
// format fmt behind settings.skipNumberOfBytes (counted in samples: include/bds_mi355x.h), read from path_in and, by the two
// conditioners, written to path_out with every byte outside the window copied through.  Plain C++, no HIP and no context: an
// error comes back as a BDS_ERR_* code with its message in the caller's buffer, the way check_args does, and the entry hands it to
// fail() behind "who: " -- except the two "Unable to ... file" messages, which stand alone as the reference words them.
// tests/host_models/record_window_check.cpp runs it under the sanitizers.
#pragma once

#include <sys/types.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "bds_mi355x.h"
#include "bds_probe_math.h"

namespace bds {

// bytes of a sample of the four formats a conditioner takes: 1, 2, 2, 4
inline int sample_bytes(int fmt) { return probe::bits_per_sample(fmt) / 8; }

// in and out must be the same buffer or disjoint ones
inline bool partial_overlap(const void *in, const void *out, size_t n_bytes) {
    const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out;
    return a != b && a < b + n_bytes && b < a + n_bytes;
}

struct RecordWindow {
    FILE *fi = nullptr, *fo = nullptr;
    const char *path_in = nullptr, *path_out = nullptr;  // the caller's strings, alive for the call
    int fmt = 0;
    int64_t skip = 0, file_bytes = 0;
    int64_t have = 0;            // samples behind `skip` samples; negative when the file ends before them
    int64_t first = 0, end = 0;  // the window's bytes in the file
    int sub = 0;                 // the window's first sample in its first byte: 1 only for a packed record that starts at a high nibble

    RecordWindow() = default;
    RecordWindow(const RecordWindow &) = delete;
    RecordWindow &operator=(const RecordWindow &) = delete;
    ~RecordWindow() {
        if (fi) std::fclose(fi);
        if (fo) std::fclose(fo);
    }

    // What a conditioner checks of its two names before it opens anything; path_out counts only when the call writes.
    static int check_names(const char *path_in, const char *path_out, bool writes, int64_t skip, char *msg, size_t len) {
        if (!path_in || (writes && !path_out)) return snprintf(msg, len, "path_in or path_out is NULL"), BDS_ERR_ARG;
        if (writes && !std::strcmp(path_in, path_out)) return snprintf(msg, len, "path_in and path_out are the same file"), BDS_ERR_ARG;
        if (skip < 0) return snprintf(msg, len, "skipNumberOfBytes < 0"), BDS_ERR_ARG;
        return BDS_OK;
    }
    // Opens the input and sizes it: `have` is set.
    int open(const char *path, int format, int64_t skip_samples, char *msg, size_t len) {
        path_in = path, fmt = format, skip = skip_samples;
        fi = std::fopen(path, "rb");
        if (!fi) return snprintf(msg, len, "Unable to read file %s", path), BDS_ERR_IO;
        std::fseek(fi, 0, SEEK_END);
        file_bytes = (int64_t)ftello(fi);
        have = probe::samples_in_bytes(fmt, (uint64_t)file_bytes) - skip;
        return BDS_OK;
    }
    // The window [skip, skip + n), n resolved by the caller: `first`, `end` and `sub` are set.
    int select(int64_t n, char *msg, size_t len) {
        if (have < 0 || n > have)
            return snprintf(msg, len, "Could not read enough data from the data file (%lld samples behind skipNumberOfBytes, %lld wanted)",
                            (long long)std::max<int64_t>(have, 0), (long long)n), BDS_ERR_ARG;
        probe::byte_span(fmt, skip, skip + std::max<int64_t>(n, 0), &first, &end);
        sub = fmt == probe::kPacked ? (int)(skip & 1) : 0;
        return BDS_OK;
    }
    // Creates the output: the entry calls this after its last argument check, so that a refused call leaves no file behind.
    int open_out(const char *path, char *msg, size_t len) {
        path_out = path;
        fo = std::fopen(path, "wb");
        return fo ? BDS_OK : (snprintf(msg, len, "Unable to write file %s", path), BDS_ERR_IO);
    }
    // n bytes from / to byte `at` of the window
    int read(int64_t at, size_t n, void *dst, char *msg, size_t len) {
        if (fseeko(fi, (off_t)(first + at), SEEK_SET) != 0 || std::fread(dst, 1, n, fi) != n) return snprintf(msg, len, "short read of %s", path_in), BDS_ERR_IO;
        return BDS_OK;
    }
    int write(int64_t at, size_t n, const void *src, char *msg, size_t len) {
        if (fseeko(fo, (off_t)(first + at), SEEK_SET) != 0 || std::fwrite(src, 1, n, fo) != n) return snprintf(msg, len, "short write on %s", path_out), BDS_ERR_IO;
        return BDS_OK;
    }
    // bytes [from, to) of the input FILE to the same place of the output, `chunk` bytes at a time
    int copy_through(int64_t from, int64_t to, char *msg, size_t len, int64_t chunk = 1 << 22) {
        std::vector<uint8_t> buf((size_t)std::min<int64_t>(std::max<int64_t>(to - from, 1), chunk));
        for (int64_t o = from; o < to; o += (int64_t)buf.size()) {
            const size_t nb = (size_t)std::min<int64_t>((int64_t)buf.size(), to - o);
            if (int rc = read(o - first, nb, buf.data(), msg, len)) return rc;
            if (int rc = write(o - first, nb, buf.data(), msg, len)) return rc;
        }
        return BDS_OK;
    }
    // what a conditioner passes on as it is: the file in front of the window with the window's first `context` bytes, and the
    // window's last `context` bytes with the file behind it
    int copy_front(int64_t context, char *msg, size_t len) { return copy_through(0, first + context, msg, len); }
    int copy_back(int64_t context, char *msg, size_t len) { return copy_through(end - context, file_bytes, msg, len); }
    // Closes both files; an output that does not close has not been written.
    int close(char *msg, size_t len) {
        if (fi) std::fclose(fi);
        FILE *out = fo;
        fi = fo = nullptr;
        return out && std::fclose(out) != 0 ? (snprintf(msg, len, "short write on %s", path_out), BDS_ERR_IO) : BDS_OK;
    }
};

}  // namespace bds
