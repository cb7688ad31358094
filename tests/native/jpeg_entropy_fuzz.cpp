// Memory safety of the JPEG host stage (memotr_amd/csrc/jpeg_entropy_core.h) on hostile input, as a stand-alone
// program for a sanitizer build:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined jpeg_entropy_fuzz.cpp
//     ./a.out <directory of .jpg streams>
// For every stream: the whole stream, 2,000 seeded single-byte corruptions of it, and -- for the two smallest streams
// -- every prefix length.  Each input is copied into a heap block of exactly its size and the outputs are heap
// blocks of exactly the size the header asks for, so a read or write one byte outside either is reported.  Errors
// RETURNED by the decoder are the expected outcome; the exit status is 0 unless a whole, unmodified stream whose name
// starts with "ok_" fails to decode.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "../../memotr_amd/csrc/jpeg_entropy_core.h"

namespace {

constexpr size_t MAX_COEF_BYTES = size_t(64) << 20;      // a corrupted header may ask for gigabytes: the decoder must refuse

struct Counts {
    long ok = 0, errors = 0;
};

int decode_copy(const uint8_t *data, size_t n, Counts &counts) {
    std::unique_ptr<uint8_t[]> in(new uint8_t[n ? n : 1]);
    memcpy(in.get(), data, n);
    char err[jpegcore::ERR_LEN];
    jpegcore::Info info;
    int rc = jpegcore::parse_header(in.get(), n, &info, err);
    if (rc == jpegcore::OK) {
        const size_t need = (size_t)info.coef_count * sizeof(int16_t);
        const size_t bytes = std::min(need, MAX_COEF_BYTES);
        std::unique_ptr<int16_t[]> coef(new int16_t[bytes / 2 + 1]);
        std::unique_ptr<uint16_t[]> qt(new uint16_t[192]);
        rc = jpegcore::decode(in.get(), n, &info, coef.get(), bytes, qt.get(), err);
        if (rc == jpegcore::OK && need > bytes) {
            fprintf(stderr, "decode accepted a buffer smaller than the image needs\n");
            return -1;
        }
    }
    if (rc != jpegcore::OK && err[0] == 0) {
        fprintf(stderr, "error code %d without a message\n", rc);
        return -1;
    }
    (rc == jpegcore::OK ? counts.ok : counts.errors)++;
    return rc;
}

uint32_t next_random(uint32_t &state) {      // xorshift32
    state ^= state << 13;
    state ^= state >> 17;
    state ^= state << 5;
    return state;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s <directory of .jpg streams>\n", argv[0]);
        return 2;
    }
    std::vector<std::pair<std::string, std::vector<uint8_t>>> streams;
    for (const auto &entry : std::filesystem::directory_iterator(argv[1])) {
        if (entry.path().extension() != ".jpg") continue;
        std::ifstream f(entry.path(), std::ios::binary);
        std::vector<uint8_t> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        streams.emplace_back(entry.path().filename().string(), std::move(bytes));
    }
    if (streams.empty()) {
        fprintf(stderr, "no .jpg streams in %s\n", argv[1]);
        return 2;
    }
    std::sort(streams.begin(), streams.end(), [](const auto &a, const auto &b) {
        return a.second.size() != b.second.size() ? a.second.size() < b.second.size() : a.first < b.first;
    });

    Counts whole, prefixes, corrupted;
    int bad = 0;
    for (size_t i = 0; i < streams.size(); ++i) {
        const std::string &name = streams[i].first;
        const std::vector<uint8_t> &s = streams[i].second;
        const int rc = decode_copy(s.data(), s.size(), whole);
        if (rc < 0 || (rc != jpegcore::OK && name.rfind("ok_", 0) == 0)) {
            fprintf(stderr, "%s: whole stream failed with %d\n", name.c_str(), rc);
            ++bad;
        }
        if (i < 2)
            for (size_t n = 0; n < s.size(); ++n)
                if (decode_copy(s.data(), n, prefixes) < 0) ++bad;
        uint32_t state = 0x9e3779b9u ^ (uint32_t)(i * 2654435761u);
        std::vector<uint8_t> m(s);
        for (int k = 0; k < 2000 && !s.empty(); ++k) {
            const size_t at = next_random(state) % s.size();
            const uint8_t keep = m[at];
            m[at] = (uint8_t)(next_random(state) >> 11);
            if (decode_copy(m.data(), m.size(), corrupted) < 0) ++bad;
            m[at] = keep;
        }
    }
    printf("streams %zu: whole ok %ld errors %ld; prefixes ok %ld errors %ld; corruptions ok %ld errors %ld\n",
           streams.size(), whole.ok, whole.errors, prefixes.ok, prefixes.errors, corrupted.ok, corrupted.errors);
    return bad ? 1 : 0;
}
