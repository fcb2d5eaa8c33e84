// exr_layers_exerciser.cpp -- the EXR data layers' shared source (csrc/rrt_exr_core.h: exr_layers_plan, exr_layers_host,
// exr_layers_header and the functions the kernels share with them) as a program of its own, for AddressSanitizer and
// UndefinedBehaviorSanitizer (tests/test_exr_layers_host.py builds it with g++ and runs it as a child process).
//
//   exr_layers_exerciser frames FILE
//     FILE holds any number of cases: a line `COMPRESSION HALF_MAX_BITS W H N_SOURCES N_CHANNELS`; per source a line
//     `WORDS KIND BOTTOM_UP` and W*H*WORDS hexadecimal words; per channel a line `NAME TYPE SOURCE WORD`.  Every plane and the
//     payload are allocated at exactly their sizes, so a read or a write past either end is reported.  Per case it prints the
//     payload and the header in hexadecimal, one line each, after checking that every filtered chunk un-filters to the chunk the
//     same layers give without compression.
//   exr_layers_exerciser refusals FILE
//     FILE is not read.  Every refusal of the plan and of the buffers' check, and the exact-fit header buffer.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../relativisticraytracer_amd/csrc/rrt_exr_core.h"

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; }    \
    } while (0)

static void defaults(rrt_exr_layers& L) {
    memset(&L, 0, sizeof(L));
    L.struct_size = sizeof(L);
    L.compression = RRT_EXR_ZIP;
    L.half_max = 65504.0f;
}

static int frames(const char* path) {
    FILE* fh = fopen(path, "r");
    if (!fh) { perror("fopen"); return 2; }
    rrt_exr_layers L;
    defaults(L);
    unsigned max_bits;
    int w, h;
    while (fscanf(fh, "%d %x %d %d %d %d", &L.compression, &max_bits, &w, &h, &L.n_sources, &L.n_channels) == 6) {
        memcpy(&L.half_max, &max_bits, 4);
        CHECK(L.n_sources >= 1 && L.n_sources <= RRT_EXR_MAX_SOURCES && L.n_channels >= 1 && L.n_channels <= RRT_EXR_MAX_CHANNELS);
        std::vector<uint32_t*> planes;
        for (int s = 0; s < L.n_sources; ++s) {
            rrt_exr_source& src = L.sources[s];
            CHECK(fscanf(fh, "%d %d %d", &src.words, &src.kind, &src.bottom_up) == 3 && src.words >= 1 && src.words <= 4);
            const size_t n = (size_t)w * h * src.words;
            uint32_t* plane = static_cast<uint32_t*>(malloc(n * 4));
            for (size_t i = 0; i < n; ++i) CHECK(fscanf(fh, "%x", &plane[i]) == 1);
            src.d_data = plane;
            planes.push_back(plane);
        }
        for (int c = 0; c < L.n_channels; ++c) {
            rrt_exr_channel& ch = L.channels[c];
            memset(&ch, 0, sizeof(ch));
            CHECK(fscanf(fh, "%31s %d %d %d", ch.name, &ch.type, &ch.source, &ch.word) == 4);
        }
        ExrLayersPlan p;
        CHECK(exr_layers_plan(&L, w, h, p) == RRT_OK);
        const size_t out_bytes = (size_t)exr_layers_bytes(p);
        uint8_t* out = static_cast<uint8_t*>(malloc(out_bytes));
        CHECK(exr_layers_host(out, &L, w, h) == RRT_OK);
        if (L.compression != RRT_EXR_NONE) {      // every chunk's inverse, into a buffer of exactly its size
            rrt_exr_layers plain = L;
            plain.compression = RRT_EXR_NONE;
            uint8_t* raw = static_cast<uint8_t*>(malloc(out_bytes));
            CHECK(exr_layers_host(raw, &plain, w, h) == RRT_OK);
            for (int y = 0; y < h; y += p.lines) {
                int y0, rows;
                size_t offset;
                exr_layer_chunk_of(p, y, y0, rows, offset);
                const size_t bytes = (size_t)rows * w * p.sum_bps;
                uint8_t* back = static_cast<uint8_t*>(malloc(bytes));
                CHECK(exr_unfilter(back, out + offset, bytes) == RRT_OK);
                CHECK(memcmp(back, raw + offset, bytes) == 0);
                free(back);
            }
            free(raw);
        }
        for (size_t i = 0; i < out_bytes; ++i) printf("%02x", out[i]);
        printf("\n");
        size_t len = 0, len2 = 0;
        uint8_t probe[2048];
        CHECK(exr_layers_header(&L, w, h, 24, 1, probe, sizeof(probe), &len) == RRT_OK);
        uint8_t* head = static_cast<uint8_t*>(malloc(len));          // an exact fit is enough
        CHECK(exr_layers_header(&L, w, h, 24, 1, head, len, &len2) == RRT_OK && len2 == len);
        for (size_t i = 0; i < len; ++i) printf("%02x", head[i]);
        printf("\n");
        free(head); free(out);
        for (uint32_t* plane : planes) free(plane);
    }
    fclose(fh);
    printf("frames ok\n");
    return 0;
}

static void channel(rrt_exr_layers& L, int c, const char* name, int type, int source, int word) {
    memset(&L.channels[c], 0, sizeof(L.channels[c]));
    snprintf(L.channels[c].name, sizeof(L.channels[c].name), "%s", name);
    L.channels[c].type = type; L.channels[c].source = source; L.channels[c].word = word;
}

static int refusals() {
    const int INVALID = RRT_ERR_INVALID_ARGUMENT;
    uint32_t* f32 = static_cast<uint32_t*>(calloc(2 * 1 * 4, 4));      // a 2 x 1 plane of 4 words
    int32_t* i32 = static_cast<int32_t*>(calloc(2 * 1, 4));            // ... and of 1
    i32[0] = -7; i32[1] = 3;
    const float px[8] = {1.5f, 0.25f, -3.0f, 1.0f, 100.0f, 2.0f, 0.75f, 1.0f};
    memcpy(f32, px, sizeof(px));
    rrt_exr_layers ok;
    defaults(ok);
    ok.compression = RRT_EXR_NONE;
    ok.n_sources = 2;
    ok.sources[0].d_data = f32; ok.sources[0].words = 4; ok.sources[0].kind = RRT_EXR_SRC_F32;
    ok.sources[1].d_data = i32; ok.sources[1].words = 1; ok.sources[1].kind = RRT_EXR_SRC_I32;
    ok.n_channels = 2;
    channel(ok, 0, "R", RRT_EXR_HALF, 0, 0);
    channel(ok, 1, "steps", RRT_EXR_UINT, 1, 0);
    ExrLayersPlan p;
    CHECK(exr_layers_plan(&ok, 2, 1, p) == RRT_OK && g_exr_err[0] == 0 && p.sum_bps == 6 && exr_layers_bytes(p) == 12 && p.n_chunks == 1);
    uint8_t* out = static_cast<uint8_t*>(malloc(12));
    CHECK(exr_layers_host(out, &ok, 2, 1) == RRT_OK);
    const uint8_t want[12] = {0x00, 0x3e, 0x40, 0x56, 0, 0, 0, 0, 3, 0, 0, 0};      // 1.5, 100 as halves; -7 -> 0; 3
    CHECK(memcmp(out, want, 12) == 0);
    rrt_exr_layers bad;
    CHECK(exr_layers_plan(nullptr, 2, 1, p) == INVALID && g_exr_err[0] != 0);
    CHECK(exr_layers_plan(&ok, 0, 1, p) == INVALID && exr_layers_plan(&ok, 2, 0, p) == INVALID);
    bad = ok; bad.struct_size -= 4; CHECK(exr_layers_plan(&bad, 2, 1, p) == INVALID);
    for (int c : {1, 4, -1}) { bad = ok; bad.compression = c; CHECK(exr_layers_plan(&bad, 2, 1, p) == INVALID); }
    for (float m : {0.0f, -1.0f, 65520.0f, 1024.5f}) { bad = ok; bad.half_max = m; CHECK(exr_layers_plan(&bad, 2, 1, p) == INVALID); }
    for (int n : {0, -1, 9}) { bad = ok; bad.n_sources = n; CHECK(exr_layers_plan(&bad, 2, 1, p) == INVALID); }
    for (int n : {0, -1, 17}) { bad = ok; bad.n_channels = n; CHECK(exr_layers_plan(&bad, 2, 1, p) == INVALID); }
    for (int n : {0, 2, 5, -1}) { bad = ok; bad.sources[0].words = n; CHECK(exr_layers_plan(&bad, 2, 1, p) == INVALID); }
    for (int k : {2, -1}) { bad = ok; bad.sources[1].kind = k; CHECK(exr_layers_plan(&bad, 2, 1, p) == INVALID); }
    for (const char* name : {"", ".R", "R.", "a b", "a-b", "a/b", "caf\xc3\xa9"}) { bad = ok; channel(bad, 0, name, RRT_EXR_HALF, 0, 0); CHECK(exr_layers_plan(&bad, 2, 1, p) == INVALID); }
    bad = ok; memset(bad.channels[0].name, 'A', 32); CHECK(exr_layers_plan(&bad, 2, 1, p) == INVALID);      // no NUL in 32 bytes
    bad = ok; memset(bad.channels[0].name, 'A', 31); CHECK(exr_layers_plan(&bad, 2, 1, p) == RRT_OK);       // 31 bytes is a name
    bad = ok; channel(bad, 0, "steps", RRT_EXR_HALF, 0, 0); CHECK(exr_layers_plan(&bad, 2, 1, p) == INVALID && strstr(g_exr_err, "\"steps\" is followed by \"steps\""));
    bad = ok; channel(bad, 0, "t", RRT_EXR_HALF, 0, 0); CHECK(exr_layers_plan(&bad, 2, 1, p) == INVALID && strstr(g_exr_err, "\"t\" is followed by \"steps\""));
    for (int t : {3, -1}) { bad = ok; bad.channels[0].type = t; CHECK(exr_layers_plan(&bad, 2, 1, p) == INVALID); }
    for (int s : {2, -1}) { bad = ok; bad.channels[0].source = s; CHECK(exr_layers_plan(&bad, 2, 1, p) == INVALID); }
    for (int k : {4, -1}) { bad = ok; bad.channels[0].word = k; CHECK(exr_layers_plan(&bad, 2, 1, p) == INVALID); }
    bad = ok; bad.channels[1].word = 1; CHECK(exr_layers_plan(&bad, 2, 1, p) == INVALID);
    bad = ok; bad.channels[0].type = RRT_EXR_UINT; CHECK(exr_layers_plan(&bad, 2, 1, p) == INVALID && strstr(g_exr_err, "UINT"));
    // a chunk of 2^31 bytes or more: 16 rows x 6 bytes x width
    bad = ok; bad.compression = RRT_EXR_ZIP;
    CHECK(exr_layers_plan(&bad, 22369622, 16, p) == INVALID && strstr(g_exr_err, "2^31") && exr_layers_plan(&bad, 22369621, 16, p) == RRT_OK);
    // the buffers: NULL, alignment, overlap
    CHECK(exr_layers_host(nullptr, &ok, 2, 1) == INVALID);
    bad = ok; bad.sources[1].d_data = nullptr; CHECK(exr_layers_host(out, &bad, 2, 1) == INVALID);
    bad = ok; bad.sources[0].d_data = reinterpret_cast<uint8_t*>(f32) + 2; CHECK(exr_layers_host(out, &bad, 2, 1) == INVALID && strstr(g_exr_err, "aligned"));
    CHECK(exr_layers_host(reinterpret_cast<uint8_t*>(f32) + 20, &ok, 2, 1) == INVALID && strstr(g_exr_err, "overlaps"));
    CHECK(exr_layers_host(reinterpret_cast<uint8_t*>(i32) + 4, &ok, 2, 1) == INVALID);                     // the second source, its last word
    CHECK(memcmp(out, want, 12) == 0 && f32[0] == 0x3fc00000u && i32[1] == 3);                             // nothing was written
    uint8_t head[2048];
    size_t len = 0, len2 = 0;
    CHECK(exr_layers_header(&ok, 2, 1, 24, 1, nullptr, 2048, &len) == INVALID && exr_layers_header(&ok, 2, 1, 24, 1, head, 2048, nullptr) == INVALID);
    CHECK(exr_layers_header(&ok, 2, 1, 0, 1, head, 2048, &len) == INVALID && exr_layers_header(&ok, 2, 1, 24, -1, head, 2048, &len) == INVALID);
    CHECK(exr_layers_header(&ok, 2, 1, 24, 1, head, 2048, &len) == RRT_OK && len > 8);
    memset(head, 0xee, sizeof(head));
    CHECK(exr_layers_header(&ok, 2, 1, 24, 1, head, len - 1, &len2) == INVALID && head[0] == 0xee);          // too small: nothing is written
    // sixteen channels with 31-byte names still fit the header's buffer
    rrt_exr_layers full = ok;
    full.n_channels = RRT_EXR_MAX_CHANNELS;
    for (int c = 0; c < RRT_EXR_MAX_CHANNELS; ++c) {
        char name[32];
        memset(name, 'a' + c, 31);
        name[31] = 0;
        channel(full, c, name, RRT_EXR_FLOAT, 0, c % 4);
    }
    CHECK(exr_layers_header(&full, 2, 1, 24, 1, head, sizeof(head), &len) == RRT_OK && len < sizeof(head));
    int32_t g[8];
    CHECK(exr_layers_plan(&ok, 2, 1, p) == RRT_OK);
    exr_layers_geometry(p, 0, g);
    CHECK(g[0] == kExrBlockX * kExrBlockY && g[6] == 0 && g[4] == 1);
    free(out); free(i32); free(f32);
    printf("refusals ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && strcmp(argv[1], "frames") == 0) return frames(argv[2]);
    if (argc == 3 && strcmp(argv[1], "refusals") == 0) return refusals();
    fprintf(stderr, "usage: exr_layers_exerciser frames|refusals FILE\n");
    return 2;
}
