// Host driver of csrc/png_inflate.h for an AddressSanitizer / UBSan build (make -C efficient-nerf_amd/csrc asan_png_decode): the decoder's
// text as the device runs it, with one lane, on zlib streams from a directory.  <dir>/manifest.txt names them, one `name H W C` per line;
// <dir>/<name>.z is the stream.  Every buffer is allocated at exactly the size the decoder is told, so that a read past the stream or a
// write past H (W C + 1) bytes is a sanitizer report.  Prints `name status adler` per stream; writes <name>.raw (the inflated bytes) and,
// where the status is 0, <name>.px (the filters undone).  tests/test_png_decode_cpu.py writes the streams and judges the output.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../efficient-nerf_amd/csrc/png_inflate.h"

static bool read_file(const std::string& path, std::vector<unsigned char>& out) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    out.resize(n > 0 ? (size_t)n : 0);
    const bool ok = out.empty() || fread(out.data(), 1, out.size(), f) == out.size();
    fclose(f);
    return ok;
}

static bool write_file(const std::string& path, const unsigned char* p, size_t n) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = n == 0 || fwrite(p, 1, n, f) == n;
    return fclose(f) == 0 && ok;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s <dir with manifest.txt and the .z streams>\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    FILE* mf = fopen((dir + "/manifest.txt").c_str(), "r");
    if (!mf) {
        fprintf(stderr, "no manifest.txt in %s\n", dir.c_str());
        return 2;
    }
    png_inflate_mem* mem = new png_inflate_mem;
    char name[256];
    unsigned H, W, C;
    int rc = 0;
    while (fscanf(mf, "%255s %u %u %u", name, &H, &W, &C) == 4) {
        std::vector<unsigned char> z;
        if (!read_file(dir + "/" + name + ".z", z) || H < 1 || W < 1 || H > 16384 || W > 16384 || C < 1 || C > 4) {
            fprintf(stderr, "%s: cannot read the stream, or a bad shape\n", name);
            rc = 2;
            break;
        }
        unsigned char* in = (unsigned char*)malloc(z.size() ? z.size() : 1);      // exactly the stream: no slack behind it
        memcpy(in, z.data(), z.size());
        const size_t n_raw = (size_t)H * (W * C + 1), n_px = (size_t)H * W * C;
        unsigned char* raw = (unsigned char*)calloc(n_raw, 1);
        uint32_t adler = 0;
        memset(mem, 0xa5, sizeof(*mem));      // nothing may depend on what an earlier stream left behind
        const int status = png_inflate(png_serial(), mem, in, (unsigned)z.size(), raw, H, W * C + 1, &adler);
        printf("%s %d %08x\n", name, status, adler);
        bool ok = write_file(dir + "/" + name + ".raw", raw, n_raw);
        if (status == R2L_PNG_OK) {
            unsigned char* px = (unsigned char*)malloc(n_px);
            png_unfilter_serial(raw, H, W, C, px);
            ok = write_file(dir + "/" + name + ".px", px, n_px) && ok;
            free(px);
        }
        free(raw);
        free(in);
        if (!ok) {
            fprintf(stderr, "%s: cannot write the results\n", name);
            rc = 2;
            break;
        }
    }
    fclose(mf);
    delete mem;
    return rc;
}
