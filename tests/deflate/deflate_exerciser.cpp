/*
 * deflate_exerciser.cpp -- the shared source of librrt_deflate.so (csrc/rrt_deflate_core.h: what rrt_deflate_host,
 * rrt_deflate_code_lengths_host and the deflate_segments kernel run) in a program of its own, for AddressSanitizer and
 * UndefinedBehaviorSanitizer: g++ -fsanitize=address,undefined, no HIP, no Python.  tests/test_deflate_host.py builds and runs it.
 *
 *   deflate_exerciser streams FILE     per case two lines "finish stream_bytes shift n" and n bytes in hex ("-" for none): prints the
 *                                      streams' sizes and their bytes in hex.  Every buffer is sized exactly (the input starts
 *                                      `shift` bytes into its allocation and ends with it), so a load or a store outside one is an error.
 *   deflate_exerciser lengths FILE     per case "limit n c0 c1 ...": prints "halvings l0 l1 ..."
 *   deflate_exerciser refusals FILE    every refusal of the two host entry points and the plan; prints nothing
 * Each ends with "<case> ok".
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../relativisticraytracer_amd/csrc/rrt_deflate_core.h"

static void check(bool ok, const char* what) {
    if (!ok) {
        fprintf(stderr, "deflate_exerciser: %s\n", what);
        exit(1);
    }
}

static int hex_digit(char c) { return c <= '9' ? c - '0' : c - 'a' + 10; }

static int streams(std::istream& in) {
    std::string head, body;
    while (std::getline(in, head) && std::getline(in, body)) {
        std::istringstream hs(head);
        int finish = 0;
        size_t stream_bytes = 0, shift = 0, n = 0;
        hs >> finish >> stream_bytes >> shift >> n;
        check(body == "-" ? n == 0 : body.size() == 2 * n, "a case's bytes do not match its size");
        uint8_t* base = n ? static_cast<uint8_t*>(malloc(shift + n)) : nullptr;      /* ends with the input's last byte */
        uint8_t* src = n ? base + shift : nullptr;
        for (size_t i = 0; i < n; ++i) src[i] = (uint8_t)(hex_digit(body[2 * i]) * 16 + hex_digit(body[2 * i + 1]));
        size_t n_streams = 0, n_segments = 0, bound = 0, scratch = 0;
        DeflatePlan p;
        check(dfl_plan(n, stream_bytes, finish, p) == RRT_OK, "plan");
        n_streams = (size_t)p.n_streams; n_segments = (size_t)p.n_segments; bound = (size_t)dfl_out_bound(p); scratch = (size_t)dfl_scratch_bytes(p);
        check(n_segments >= n_streams && scratch > bound, "plan sizes");
        std::vector<uint8_t> out(bound);
        std::vector<uint32_t> sizes(n_streams);
        size_t total = 0;
        check(dfl_host(out.data(), sizes.data(), src, n, stream_bytes, finish, &total) == RRT_OK, g_dfl_err);
        check(total <= bound, "total beyond out_bound");
        for (size_t j = 0; j < n_streams; ++j) printf("%s%u", j ? " " : "", sizes[j]);
        printf("\n");
        for (size_t i = 0; i < total; ++i) printf("%02x", out[i]);
        printf("\n");
        free(base);
    }
    return 0;
}

static int lengths(std::istream& in) {
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        int limit = 0, n = 0;
        ls >> limit >> n;
        std::vector<uint32_t> counts((size_t)n);
        for (int i = 0; i < n; ++i) ls >> counts[(size_t)i];
        std::vector<uint8_t> out((size_t)n);
        int32_t halvings = -1;
        check(dfl_code_lengths(counts.data(), n, limit, out.data(), &halvings) == RRT_OK, g_dfl_err);
        printf("%d", halvings);
        for (int i = 0; i < n; ++i) printf(" %d", out[(size_t)i]);
        printf("\n");
    }
    return 0;
}

static int refusals() {
    uint8_t src[64] = {0}, out[128];
    uint32_t sizes[8];
    const int bad = RRT_ERR_INVALID_ARGUMENT;
    check(dfl_host(nullptr, sizes, src, 4, 4, 1, nullptr) == bad && strstr(g_dfl_err, "NULL"), "out NULL");
    check(dfl_host(out, nullptr, src, 4, 4, 1, nullptr) == bad, "sizes NULL");
    check(dfl_host(out, sizes, nullptr, 4, 4, 1, nullptr) == bad, "src NULL");
    check(dfl_host(out, sizes, nullptr, 0, 4, 1, nullptr) == RRT_OK && g_dfl_err[0] == 0, "an empty input needs no src");
    check(dfl_host(out, sizes, src, 4, 0, 1, nullptr) == bad && strstr(g_dfl_err, "stream_bytes"), "stream_bytes 0");
    check(dfl_host(out, sizes, src, 4, 4, 2, nullptr) == bad && strstr(g_dfl_err, "finish"), "finish 2");
    check(dfl_host(out, sizes, src, (size_t)1 << 32, 4, 1, nullptr) == bad && strstr(g_dfl_err, "2^32"), "n 2^32");
    check(dfl_host(out, sizes, src, 400000000u, 1, 1, nullptr) == bad && strstr(g_dfl_err, "out_bound"), "out_bound 2^32");
    check(dfl_host(src + 8, sizes, src, 16, 16, 1, nullptr) == bad && strstr(g_dfl_err, "overlaps"), "out over src");
    check(dfl_host(out, reinterpret_cast<uint32_t*>(out + 8), src, 16, 16, 1, nullptr) == bad && strstr(g_dfl_err, "overlap"), "sizes over out");
    check(dfl_host(out, reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(sizes) + 2), src, 4, 4, 1, nullptr) == bad && strstr(g_dfl_err, "aligned"), "sizes misaligned");
    uint32_t counts[4] = {1, 2, 3, 4};
    uint8_t lens[4];
    check(dfl_code_lengths(nullptr, 4, 7, lens, nullptr) == bad, "counts NULL");
    check(dfl_code_lengths(counts, 1, 7, lens, nullptr) == bad, "one symbol");
    check(dfl_code_lengths(counts, 4, 1, lens, nullptr) == bad, "a limit too small for the alphabet");
    check(dfl_code_lengths(counts, 4, 16, lens, nullptr) == bad, "limit 16");
    check(dfl_code_lengths(counts, 4, 7, lens, nullptr) == RRT_OK, "lengths");
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const std::string what = argv[1];
    std::ifstream in(argv[2]);
    int rc = 2;
    if (what == "streams") rc = streams(in);
    else if (what == "lengths") rc = lengths(in);
    else if (what == "refusals") rc = refusals();
    if (rc == 0) printf("%s ok\n", what.c_str());
    return rc;
}
