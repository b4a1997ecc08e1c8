// csrc/bds_record_window.h in a stand-alone program, so that it can run under the sanitizers (tests/test_record_window_cases.py
// compiles it with -fsanitize=address,undefined).  No arithmetic of its own.  Lines on stdin ("-" is a NULL name), one output
// line each, "rc|...|message":
//   N path_in path_out writes skip -> check_names
//   O path fmt skip                -> a new window, open: rc|have|file_bytes|message
//   S n                            -> select: rc|first_byte|end_byte|sub|message
//   W path                         -> open_out
//   C from to chunk                -> copy_through (chunk 0: the default)
//   F context / B context          -> copy_front / copy_back
//   R window_byte n                -> read: rc|the bytes in hex|message
//   X window_byte hex              -> write
//   K                              -> close
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "bds_blank_math.h"
#include "bds_notch_math.h"
#include "bds_record_window.h"

int main() {
    std::unique_ptr<bds::RecordWindow> w(new bds::RecordWindow);
    std::vector<std::string> names;  // the window keeps the caller's strings
    names.reserve(4096);
    char line[4096], a[2048], b[2048], msg[1024];
    while (std::fgets(line, sizeof line, stdin)) {
        msg[0] = 0;
        long long x = 0, y = 0, z = 0;
        int i = 0;
        if (line[0] == 'N' && std::sscanf(line + 1, "%2047s %2047s %d %lld", a, b, &i, &x) == 4) {
            const int rc = bds::RecordWindow::check_names(std::strcmp(a, "-") ? a : nullptr, std::strcmp(b, "-") ? b : nullptr, i != 0, x, msg, sizeof msg);
            std::printf("%d|%s\n", rc, msg);
        } else if (line[0] == 'O' && std::sscanf(line + 1, "%2047s %d %lld", a, &i, &x) == 3) {
            w.reset(new bds::RecordWindow);
            names.emplace_back(a);
            const int rc = w->open(names.back().c_str(), i, x, msg, sizeof msg);
            std::printf("%d|%lld|%lld|%s\n", rc, (long long)w->have, (long long)w->file_bytes, msg);
        } else if (line[0] == 'S' && std::sscanf(line + 1, "%lld", &x) == 1) {
            const int rc = w->select(x, msg, sizeof msg);
            std::printf("%d|%lld|%lld|%d|%s\n", rc, (long long)w->first, (long long)w->end, w->sub, msg);
        } else if (line[0] == 'W' && std::sscanf(line + 1, "%2047s", a) == 1) {
            names.emplace_back(a);
            const int rc = w->open_out(names.back().c_str(), msg, sizeof msg);
            std::printf("%d|%s\n", rc, msg);
        } else if (line[0] == 'C' && std::sscanf(line + 1, "%lld %lld %lld", &x, &y, &z) == 3) {
            const int rc = z ? w->copy_through(x, y, msg, sizeof msg, z) : w->copy_through(x, y, msg, sizeof msg);
            std::printf("%d|%s\n", rc, msg);
        } else if ((line[0] == 'F' || line[0] == 'B') && std::sscanf(line + 1, "%lld", &x) == 1) {
            const int rc = line[0] == 'F' ? w->copy_front(x, msg, sizeof msg) : w->copy_back(x, msg, sizeof msg);
            std::printf("%d|%s\n", rc, msg);
        } else if (line[0] == 'R' && std::sscanf(line + 1, "%lld %lld", &x, &y) == 2) {
            std::vector<unsigned char> buf((size_t)y);
            const int rc = w->read(x, (size_t)y, buf.data(), msg, sizeof msg);
            std::printf("%d|", rc);
            for (size_t k = 0; k < buf.size() && !rc; ++k) std::printf("%02x", buf[k]);
            std::printf("|%s\n", msg);
        } else if (line[0] == 'X' && std::sscanf(line + 1, "%lld %2047s", &x, a) == 2) {
            std::vector<unsigned char> buf(std::strlen(a) / 2);
            for (size_t k = 0; k < buf.size(); ++k) {
                unsigned v = 0;
                std::sscanf(a + 2 * k, "%2x", &v);
                buf[k] = (unsigned char)v;
            }
            const int rc = w->write(x, buf.size(), buf.data(), msg, sizeof msg);
            std::printf("%d|%s\n", rc, msg);
        } else if (line[0] == 'K') {
            const int rc = w->close(msg, sizeof msg);
            std::printf("%d|%s\n", rc, msg);
        } else {
            return 2;
        }
    }
    // what moved out of the conditioners' headers is the one definition both see
    const char probe[8] = {0};
    if (bds::sample_bytes(bds::probe::kS16C) != 4 || bds::partial_overlap(probe, probe, 8) || !bds::partial_overlap(probe, probe + 1, 8) ||
        bds::partial_overlap(probe, probe + 4, 4))
        return 3;
    return 0;
}
