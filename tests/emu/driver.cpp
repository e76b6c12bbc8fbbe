// Stand-alone driver of the emulated tests (tests/emu_case.py writes its input and reads its output).
//   driver query ENTRY a b c ...     prints the value of a size function called with integer arguments
//   driver run CASEFILE              runs one case
// A case file holds one statement per line:
//   entry NAME
//   config WG_DESCENDING THREADS_DESCENDING LDS_POISON GLOBAL_POISON
//   buf NAME FILE BYTES SKEW PAY_LO PAY_HI CHUNK   the image FILE of BYTES bytes goes to a heap block of SKEW + BYTES bytes that is
//                                     256-byte aligned, at offset SKEW: its last byte is the block's last, so that a sanitizer's
//                                     red zone starts right behind it; the SKEW bytes in front hold GLOBAL_POISON.  CHUNK = 1
//                                     registers [PAY_LO, PAY_HI) of the image as the payload of an input whose reader may load
//                                     the 16-byte blocks around it (the streaming loads then check that a block holds payload)
//   arg p NAME OFFSET | arg v INTEGER one argument of the entry, in order: a pointer into a buffer's image, or an integer (for a
//                                     float or double parameter: the bits of a float32)
// After the call every block (SKEW bytes and image) is written to FILE.out, and "rc", "misaligned" and "nopayload" are printed.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include <map>
#include <type_traits>
#include <utility>
#include "v3d_common.h"
#include EMU_ENTRY_HEADER

typedef std::vector<unsigned long long> Args;
template <class T> static T conv(unsigned long long v)
{
    if constexpr (std::is_pointer<T>::value) return reinterpret_cast<T>((uintptr_t)v);
    else if constexpr (std::is_floating_point<T>::value) { const uint32_t b = (uint32_t)v; float f; memcpy(&f, &b, 4); return (T)f; }   // a float32's bits
    else return static_cast<T>((long long)v);
}
template <class R, class... A, size_t... I> static long long call_idx(R (*fn)(A...), const Args& a, std::index_sequence<I...>)
{
    return (long long)fn(conv<A>(a[I])...);
}
template <class R, class... A> static long long call(R (*fn)(A...), const Args& a)
{
    if (a.size() != sizeof...(A)) { fprintf(stderr, "driver: %zu arguments given, the entry takes %zu\n", a.size(), sizeof...(A)); exit(2); }
    return call_idx(fn, a, std::index_sequence_for<A...>{});
}
static bool dispatch(const std::string& name, const Args& a, long long* rc)
{
#define E(fn) if (name == #fn) { *rc = call(fn, a); return true; }
    EMU_ENTRIES
#undef E
    return false;
}

struct Buf { std::string file; unsigned char* block; size_t bytes, skew; };

int main(int argc, char** argv)
{
    if (argc >= 3 && !strcmp(argv[1], "query")) {
        Args a; for (int i = 3; i < argc; i++) a.push_back(strtoull(argv[i], nullptr, 0));
        long long rc;
        if (!dispatch(argv[2], a, &rc)) { fprintf(stderr, "driver: unknown entry %s\n", argv[2]); return 2; }
        printf("%lld\n", rc);
        return 0;
    }
    if (argc != 3 || strcmp(argv[1], "run")) { fprintf(stderr, "usage: driver run CASEFILE | driver query ENTRY ARGS\n"); return 2; }
    FILE* cf = fopen(argv[2], "r");
    if (!cf) { perror(argv[2]); return 2; }
    std::string entry; Args args; std::map<std::string, Buf> bufs; int gpoison = 0xA5;
    char line[4096];
    while (fgets(line, sizeof line, cf)) {
        char kw[32], s1[1024], s2[2048]; long long v[5];
        if (sscanf(line, "%31s", kw) != 1) continue;
        if (!strcmp(kw, "entry") && sscanf(line, "%*s %1023s", s1) == 1) entry = s1;
        else if (!strcmp(kw, "config") && sscanf(line, "%*s %lld %lld %lld %lld", v, v + 1, v + 2, v + 3) == 4) { emu_configure((int)v[0], (int)v[1], (int)v[2]); gpoison = (int)v[3]; }
        else if (!strcmp(kw, "buf") && sscanf(line, "%*s %1023s %2047s %lld %lld %lld %lld %lld", s1, s2, v, v + 1, v + 2, v + 3, v + 4) == 7) {
            Buf b; b.file = s2; b.bytes = (size_t)v[0]; b.skew = (size_t)v[1];
            void* p = nullptr;
            if (posix_memalign(&p, 256, b.skew + b.bytes)) { fprintf(stderr, "driver: out of memory\n"); return 2; }
            b.block = (unsigned char*)p;
            memset(b.block, gpoison, b.skew);
            FILE* f = fopen(s2, "rb");
            if (!f || fread(b.block + b.skew, 1, b.bytes, f) != b.bytes) { fprintf(stderr, "driver: cannot read %zu bytes of %s\n", b.bytes, s2); return 2; }
            fclose(f);
            if (v[4]) emu_register_payload(b.block + b.skew, b.bytes, b.block + b.skew + v[2], (size_t)(v[3] - v[2]));
            bufs[s1] = b;
        }
        else if (!strcmp(kw, "arg") && sscanf(line, "%*s %1023s", s1) == 1 && !strcmp(s1, "p") && sscanf(line, "%*s %*s %1023s %lld", s1, v) == 2) {
            if (!bufs.count(s1)) { fprintf(stderr, "driver: unknown buffer %s\n", s1); return 2; }
            const Buf& b = bufs[s1];
            args.push_back((unsigned long long)(uintptr_t)(b.block + b.skew + v[0]));
        }
        else if (!strcmp(kw, "arg") && !strcmp(s1, "v") && sscanf(line, "%*s %*s %lld", v) == 1) args.push_back((unsigned long long)v[0]);
        else { fprintf(stderr, "driver: bad line: %s", line); return 2; }
    }
    fclose(cf);
    long long rc;
    if (!dispatch(entry, args, &rc)) { fprintf(stderr, "driver: unknown entry %s\n", entry.c_str()); return 2; }
    for (auto& kv : bufs) {
        const Buf& b = kv.second;
        FILE* f = fopen((b.file + ".out").c_str(), "wb");
        if (!f || fwrite(b.block, 1, b.skew + b.bytes, f) != b.skew + b.bytes) { fprintf(stderr, "driver: cannot write %s.out\n", b.file.c_str()); return 2; }
        fclose(f);
        free(b.block);
    }
    printf("rc %lld\nmisaligned %d\nnopayload %d\n", rc, emu_misaligned_loads(), emu_nopayload_loads());
    return 0;
}
