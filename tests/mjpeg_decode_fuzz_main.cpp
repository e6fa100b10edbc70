// Stand-alone driver of the host half of the JPEG decoder (csrc/mjpeg_parse.hip, which is plain C++) for the address / undefined-
// behaviour sanitizers: tests/test_mjpeg_decode_cpu.py builds both with -fsanitize=address,undefined and runs the corrupt streams
// through them.  Every buffer is a heap block of exactly the size the library asks for, so a byte read or written past one is caught.
//   mjpeg_decode_fuzz FILE...      each FILE: u32 count, then per stream u32 length + bytes.  Prints "parsed unsupported corrupt undecodable".
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

extern "C" {
int stabnet_mjpeg_parse(const unsigned char* jpeg, size_t nbytes, int* info16, unsigned char* blob, size_t blob_cap);
int stabnet_mjpeg_entropy_host(const unsigned char* jpeg, size_t nbytes, const unsigned char* blob, size_t blob_bytes, short* coef,
                               size_t coef_count);
}

void stabnet_set_error(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
}

int main(int argc, char** argv) {
    long ok = 0, unsupported = 0, corrupt = 0, undecodable = 0;
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
            int rc = stabnet_mjpeg_parse(jpeg, len, info, nullptr, 0);
            if (rc == 0) {
                unsigned char* blob = static_cast<unsigned char*>(malloc((size_t)info[9]));
                short* coef = static_cast<short*>(malloc((size_t)info[11] * 64 * sizeof(short)));
                rc = stabnet_mjpeg_parse(jpeg, len, info, blob, (size_t)info[9]);
                if (rc != 0) { fprintf(stderr, "the second parse disagrees with the first\n"); return 3; }
                if (stabnet_mjpeg_entropy_host(jpeg, len, blob, (size_t)info[9], coef, (size_t)info[11] * 64) == 0) ++ok; else ++undecodable;
                free(coef);
                free(blob);
            } else if (rc == 1) {
                ++unsupported;
            } else {
                ++corrupt;
            }
            free(jpeg);
        }
        fclose(f);
    }
    printf("%ld %ld %ld %ld\n", ok, unsupported, corrupt, undecodable);
    return 0;
}
