// Memory safety and output of the JPEG encoder's host stage (memotr_amd/csrc/jpeg_encode_core.h), as a stand-alone
// program for a sanitizer build:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined jpeg_encode_check.cpp
//     ./a.out <directory>
// The directory holds pairs <name>.coef / <name>.jpg.  A .coef file is int32 width, height, hmax followed by the
// frame's coef_count int16 coefficients and 192 uint16 table words; the .jpg is the stream they must give.  For every
// pair: the size query (no buffer), the stream into a heap block of exactly its size (compared with the .jpg), and
// into heap blocks that are too small -- one byte short, and every capacity below 700 bytes (inside the header) for
// the first pair -- which must return the same size and, the blocks being exact, cannot write past the end unseen.
// Then 20 seeded sets of arbitrary int16 "coefficients" per pair: the encoder must return a size or refuse (-3).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "../../memotr_amd/csrc/jpeg_encode_core.h"

namespace {

std::vector<uint8_t> slurp(const std::filesystem::path &p) {
    std::ifstream f(p, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int64_t encode_exact(const int16_t *coef, const uint16_t *qt, const jpegenc::Info &info, size_t cap,
                     std::vector<uint8_t> *keep) {
    std::unique_ptr<uint8_t[]> out(new uint8_t[cap ? cap : 1]);
    const int64_t n = jpegenc::encode(coef, qt, &info, cap ? out.get() : nullptr, cap);
    if (keep && n >= 0 && (size_t)n <= cap) keep->assign(out.get(), out.get() + n);
    return n;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s <directory of .coef / .jpg pairs>\n", argv[0]);
        return 2;
    }
    std::vector<std::filesystem::path> sets;
    for (const auto &e : std::filesystem::directory_iterator(argv[1]))
        if (e.path().extension() == ".coef") sets.push_back(e.path());
    std::sort(sets.begin(), sets.end());
    long equal = 0, short_ok = 0, refused = 0, sized = 0;
    uint32_t seed = 12345;
    bool first = true;
    for (const auto &p : sets) {
        const std::vector<uint8_t> raw = slurp(p);
        std::filesystem::path jp = p;
        const std::vector<uint8_t> want = slurp(jp.replace_extension(".jpg"));
        int32_t head[3];
        if (raw.size() < sizeof(head)) { fprintf(stderr, "%s: too short\n", p.c_str()); return 1; }
        memcpy(head, raw.data(), sizeof(head));
        jpegenc::Info info;
        if (jpegenc::geometry(head[0], head[1], head[2], &info)) { fprintf(stderr, "%s: bad geometry\n", p.c_str()); return 1; }
        const size_t words = (size_t)info.coef_count + 192;
        if (raw.size() != sizeof(head) + 2 * words) { fprintf(stderr, "%s: size does not match\n", p.c_str()); return 1; }
        std::unique_ptr<int16_t[]> coef(new int16_t[info.coef_count]);      // exact heap blocks: overreads are seen
        std::unique_ptr<uint16_t[]> qt(new uint16_t[192]);
        memcpy(coef.get(), raw.data() + sizeof(head), 2 * (size_t)info.coef_count);
        memcpy(qt.get(), raw.data() + sizeof(head) + 2 * (size_t)info.coef_count, 2 * 192);

        const int64_t n = encode_exact(coef.get(), qt.get(), info, 0, nullptr);
        if (n != (int64_t)want.size()) {
            fprintf(stderr, "%s: size query gave %lld, the stream has %zu bytes\n", p.c_str(), (long long)n, want.size());
            return 1;
        }
        std::vector<uint8_t> got;
        if (encode_exact(coef.get(), qt.get(), info, (size_t)n, &got) != n || got != want) {
            fprintf(stderr, "%s: the stream differs from the .jpg\n", p.c_str());
            return 1;
        }
        ++equal;
        std::vector<size_t> caps = {(size_t)n - 1, (size_t)n / 2, 1};
        if (first)
            for (size_t c = 2; c < 700 && c < (size_t)n; ++c) caps.push_back(c);
        first = false;
        for (size_t cap : caps) {
            std::vector<uint8_t> part;
            std::unique_ptr<uint8_t[]> out(new uint8_t[cap]);
            if (jpegenc::encode(coef.get(), qt.get(), &info, out.get(), cap) != n) {
                fprintf(stderr, "%s: capacity %zu did not return the size needed\n", p.c_str(), cap);
                return 1;
            }
            if (memcmp(out.get(), want.data(), cap) != 0) {
                fprintf(stderr, "%s: capacity %zu: the bytes that fit differ\n", p.c_str(), cap);
                return 1;
            }
            ++short_ok;
        }
        for (int k = 0; k < 20; ++k) {
            for (int64_t i = 0; i < info.coef_count; ++i) {
                seed = seed * 1664525u + 1013904223u;
                // mostly zeros and small values, now and then anything at all
                const uint32_t r = seed >> 8;
                coef[i] = (r & 7) ? (int16_t)0 : ((r & 0x3F8) ? (int16_t)((int)(r >> 10 & 2047) - 1023) : (int16_t)(r >> 8));
            }
            const int64_t m = encode_exact(coef.get(), qt.get(), info, k & 1 ? 4096 : 0, nullptr);
            if (m == -3) ++refused;
            else if (m > 0) ++sized;
            else { fprintf(stderr, "%s: arbitrary coefficients returned %lld\n", p.c_str(), (long long)m); return 1; }
        }
    }
    // arguments the encoder refuses
    jpegenc::Info info;
    uint16_t qt[192];
    int16_t zero[3 * 64] = {0};
    if (jpegenc::geometry(8, 8, 3, &info) != 1 || jpegenc::geometry(0, 8, 1, &info) != 1 ||
        jpegenc::quant_tables(0, qt) != 1 || jpegenc::quant_tables(101, qt) != 1 || jpegenc::quant_tables(75, qt) != 0 ||
        jpegenc::geometry(8, 8, 1, &info) != 0) {
        fprintf(stderr, "argument checks\n");
        return 1;
    }
    info.mcus_x = 2;
    if (jpegenc::encode(zero, qt, &info, nullptr, 0) != -1) { fprintf(stderr, "a broken geometry was accepted\n"); return 1; }
    jpegenc::geometry(8, 8, 1, &info);
    qt[5] = 256;
    if (jpegenc::encode(zero, qt, &info, nullptr, 0) != -2) { fprintf(stderr, "a 9-bit table entry was accepted\n"); return 1; }
    printf("sets %zu: equal %ld; short buffers ok %ld; arbitrary coefficients sized %ld refused %ld\n", sets.size(), equal,
           short_ok, sized, refused);
    return 0;
}
