// loader_prefixes_main.cpp -- parse_scene over every case text of tests/_loader_cases.py and over
// every prefix of each (a truncation at any byte), each input in a heap buffer of exactly its size,
// so that a read past the end is seen; the stretch cuts too: the cuts of every input, every case
// parsed in 16 stretches, and a text over 1 MiB made of all the cases at parse_scene's own
// choice and in 2, 3 and 16 stretches, whole and cut short by 1 .. 8 bytes.  Built with -fsanitize=address,undefined and run as a
// child process by tests/test_loader_host.py; never loaded into Python, never run on a GPU.
//   loader_prefixes <blob>     blob: u32 n, then n x (u32 len, bytes)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "host/pt_scene.h"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<unsigned char> blob;
    unsigned char tmp[65536];
    for (size_t k; (k = fread(tmp, 1, sizeof tmp, f)) > 0;) blob.insert(blob.end(), tmp, tmp + k);
    fclose(f);
    if (blob.size() < 4) return 2;
    uint32_t n;
    memcpy(&n, blob.data(), 4);
    size_t at = 4, inputs = 0, prims = 0;
    // (the warnings of thousands of truncated command names; the sanitizers' reports, which go to
    // file descriptor 2 and not through this stream, stay)
    if (!freopen("/dev/null", "w", stderr)) return 2;
    std::vector<char> all;
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t len;
        if (at + 4 > blob.size()) return 2;
        memcpy(&len, blob.data() + at, 4);
        at += 4;
        if (at + len > blob.size()) return 2;
        for (uint32_t k = 0; k <= len; ++k) {
            char* buf = static_cast<char*>(malloc(k ? k : 1));
            if (k) memcpy(buf, blob.data() + at, k);
            pth::HScene S;
            pth::parse_scene(k ? buf : nullptr, k, S);
            prims += S.prims.size();
            ++inputs;
            // the cuts of every input (no threads: those cost more than the parse here), the
            // whole text also parsed in them
            const std::vector<size_t> cut = pth::scene_stretch_cuts(k ? buf : nullptr, k, 4);
            if (cut.front() != 0 || cut.back() != k) return 3;
            if (k == len) {
                pth::HScene S2;
                pth::parse_scene_stretches(k ? buf : nullptr, k, S2, 16);
                if (S2.prims.size() != S.prims.size() || S2.warnings != S.warnings) return 3;
            }
            free(buf);
        }
        all.insert(all.end(), blob.begin() + at, blob.begin() + at + len);
        all.push_back('\n');
        all.push_back('\n');
        at += len;
    }
    // over 1 MiB: parse_scene's own stretches, and given numbers of them
    std::vector<char> big;
    while (big.size() <= (1u << 20) + 4096) big.insert(big.end(), all.begin(), all.end());
    size_t want = 0;
    for (unsigned T : {0u, 1u, 2u, 3u, 16u}) {
        for (size_t cut = 0; cut <= (T == 16 ? 8u : 0u); ++cut) {
            const size_t k = big.size() - cut;
            char* buf = static_cast<char*>(malloc(k));
            memcpy(buf, big.data(), k);
            pth::HScene S;
            if (T) pth::parse_scene_stretches(buf, k, S, T);
            else pth::parse_scene(buf, k, S);
            if (cut == 0 && T == 0) want = S.prims.size();
            if (cut == 0 && S.prims.size() != want) return 3;
            prims += S.prims.size();
            ++inputs;
            free(buf);
        }
    }
    printf("inputs=%zu prims=%zu\n", inputs, prims);
    return 0;
}
