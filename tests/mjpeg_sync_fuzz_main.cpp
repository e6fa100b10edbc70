// Stand-alone driver of the host twin of the parallel entropy back end (stabnet_mjpeg_entropy_sync_host in csrc/mjpeg_parse.hip, which
// is plain C++ and runs the walks of csrc/jpeg_sync.h) for the address / undefined-behaviour sanitizers: tests/test_mjpeg_sync_cpu.py
// builds both with -fsanitize=address,undefined and runs the corrupt streams through them.  Every buffer is a heap block of exactly
// the size the library asks for, so a byte read or written past one is caught.  A run must be refused or give the coefficients of
// the sequential routine.
//   mjpeg_sync_fuzz FILE...      each FILE: u32 count, then per stream u32 length + bytes.  Prints "runs same refused skipped".
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

extern "C" {
int stabnet_mjpeg_parse(const unsigned char* jpeg, size_t nbytes, int* info16, unsigned char* blob, size_t blob_cap);
int stabnet_mjpeg_entropy_host(const unsigned char* jpeg, size_t nbytes, const unsigned char* blob, size_t blob_bytes, short* coef,
                               size_t coef_count);
int stabnet_mjpeg_entropy_sync_host(const unsigned char* jpeg, size_t nbytes, const unsigned char* blob, size_t blob_bytes, short* coef,
                                    size_t coef_count, int chunk_bytes, int rounds, int* stats);
}

void stabnet_set_error(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
}

int main(int argc, char** argv) {
    static const int kCases[][2] = {{1, 1}, {2, 0}, {4, 8}, {16, 1}, {64, 8}, {4096, 0}};       // chunk_bytes, rounds
    long runs = 0, same = 0, refused = 0, skipped = 0;
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        unsigned count = 0;
        if (fread(&count, 4, 1, f) != 1) return 2;
        for (unsigned s = 0; s < count; ++s) {
            unsigned len = 0;
            if (fread(&len, 4, 1, f) != 1) return 2;
            unsigned char* jpeg = static_cast<unsigned char*>(malloc(len ? len : 1));
            if (len && fread(jpeg, 1, len, f) != len) return 2;
            int info[16];
            if (stabnet_mjpeg_parse(jpeg, len, info, nullptr, 0) != 0 || info[5] != 1) {
                ++skipped;
                free(jpeg);
                continue;
            }
            const size_t ncoef = (size_t)info[11] * 64;
            unsigned char* blob = static_cast<unsigned char*>(malloc((size_t)info[9]));
            short* ref = static_cast<short*>(malloc(ncoef * sizeof(short)));
            if (stabnet_mjpeg_parse(jpeg, len, info, blob, (size_t)info[9]) != 0) { fprintf(stderr, "the second parse disagrees with the first\n"); return 3; }
            const int href = stabnet_mjpeg_entropy_host(jpeg, len, blob, (size_t)info[9], ref, ncoef);
            for (const auto& c : kCases) {
                short* coef = static_cast<short*>(malloc(ncoef * sizeof(short)));
                int stats[2] = {-1, -1};
                const int rc = stabnet_mjpeg_entropy_sync_host(jpeg, len, blob, (size_t)info[9], coef, ncoef, c[0], c[1], stats);
                ++runs;
                if (rc != 0) {
                    ++refused;
                } else {
                    if (href != 0 || memcmp(coef, ref, ncoef * sizeof(short)) != 0) {
                        fprintf(stderr, "stream %u, chunk %d, rounds %d: accepted, but not the sequential routine's coefficients\n", s, c[0], c[1]);
                        return 3;
                    }
                    ++same;
                }
                if (href != 0 && rc == 0) return 3;
                free(coef);
            }
            free(ref);
            free(blob);
            free(jpeg);
        }
        fclose(f);
    }
    printf("%ld %ld %ld %ld\n", runs, same, refused, skipped);
    return 0;
}
