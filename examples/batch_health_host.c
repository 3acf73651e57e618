/* Which request of a batch went non-finite, from a host that is not Python: loads a plan file exported with per-image health
 * (python -m img2img_turbo_amd.plan_file --health stages|all --health-per-image ...), runs it, and prints one line per request.
 *
 *     cc -O2 -I include examples/batch_health_host.c -o batch_health_host -L img2img-turbo_amd/csrc -li2i_turbo -Wl,-rpath,img2img-turbo_amd/csrc
 *     ./batch_health_host pix2pix_bs8_512_health.i2iplan x.bin ctx.bin eps.bin [runs]
 *
 * "verdict" holds one row of four uint32 per image (include/i2i_turbo.h, i2i_scan_verdict_params: first_bad, first_over, runs, bad_runs),
 * written by the program's last op: first_bad = 1 + the index of the first tap, in program order, at which THAT image held a NaN or an Inf
 * in the most recent run (0 = none), first_over the same for finite values over the limit; runs / bad_runs count since the file was loaded.
 * "health_names" holds the tap labels, each NUL-terminated; "health" (not read here) the taps x B x 8 uint64 records behind the verdict.
 * Nothing in the forward mixes images, so the requests whose row says 0 are good whatever happened to their neighbours.
 * Exit status: 0 = every request finite in the last run, 3 = some request was not, 1 / 2 = errors.  tests/test_health_batch_emu.py builds
 * this file with gcc against the CPU emulator library. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "i2i_turbo.h"

static int fail(const char* what) {
    fprintf(stderr, "batch_health_host: %s: %s\n", what, i2i_last_error());
    return 1;
}

static int feed(void* plan, const char* name, const char* path) {
    void* dev;
    size_t bytes;
    if (i2i_plan_io(plan, name, &dev, &bytes) != I2I_OK) return fail(name);
    void* host = malloc(bytes);
    FILE* f = fopen(path, "rb");
    if (!host || !f || fread(host, 1, bytes, f) != bytes) { fprintf(stderr, "batch_health_host: %s: cannot read %zu bytes from %s\n", name, bytes, path); return 1; }
    fclose(f);
    const int rc = i2i_plan_write(plan, name, host, bytes);
    free(host);
    return rc == I2I_OK ? 0 : fail(name);
}

/* label of tap `index` (0-based) in the NUL-separated list, or "?" behind its end */
static const char* label_of(const char* names, size_t name_bytes, uint32_t index) {
    const char* label = names;
    for (uint32_t t = 0; t < index && label < names + name_bytes; ++t) label += strlen(label) + 1;
    return label < names + name_bytes ? label : "?";
}

int main(int argc, char** argv) {
    if (argc < 5) { fprintf(stderr, "usage: %s plan x.bin ctx.bin eps.bin [runs]\n", argv[0]); return 2; }
    if (i2i_abi_version() != I2I_ABI_VERSION) { fprintf(stderr, "batch_health_host: header / library ABI mismatch\n"); return 2; }
    const int runs = argc > 5 ? atoi(argv[5]) : 1;
    void* plan = NULL;
    if (i2i_plan_load(argv[1], &plan) != I2I_OK) return fail("load");
    void* dev;
    size_t verdict_bytes, rec_bytes, name_bytes, eps_bytes;
    if (i2i_plan_io(plan, "verdict", &dev, &verdict_bytes) != I2I_OK || i2i_plan_io(plan, "health", &dev, &rec_bytes) != I2I_OK ||
        i2i_plan_io(plan, "health_names", &dev, &name_bytes) != I2I_OK) {
        fprintf(stderr, "batch_health_host: %s carries no per-image health (export it with --health stages|all --health-per-image)\n", argv[1]);
        return 2;
    }
    /* the batch size: "eps" is fp32 [B][4][H/8][W/8], "out" B images -- but the file says it directly: one 16-byte verdict row per image,
     * and "health" holds a whole number of taps of B records each */
    const size_t B = verdict_bytes / 16;
    if (B < 1 || verdict_bytes != 16 * B || rec_bytes % (64 * B) != 0) {
        fprintf(stderr, "batch_health_host: \"verdict\" holds %zu bytes and \"health\" %zu: expected 16 * B and taps * B * 64\n", verdict_bytes, rec_bytes);
        return 2;
    }
    if (i2i_plan_io(plan, "eps", &dev, &eps_bytes) != I2I_OK) return fail("eps");
    if (eps_bytes % B != 0) { fprintf(stderr, "batch_health_host: \"eps\" (%zu bytes) is not %zu images\n", eps_bytes, B); return 2; }
    const size_t n_taps = rec_bytes / (64 * B);
    if (feed(plan, "x", argv[2]) || feed(plan, "ctx", argv[3]) || feed(plan, "eps", argv[4])) return 1;
    for (int i = 0; i < runs; ++i)
        if (i2i_plan_run(plan, NULL) != I2I_OK) return fail("run");
    uint32_t* verdict = (uint32_t*)malloc(verdict_bytes);
    char* names = (char*)malloc(name_bytes + 1);
    if (!verdict || !names) return 1;
    if (i2i_plan_read(plan, "verdict", verdict, verdict_bytes) != I2I_OK || i2i_plan_read(plan, "health_names", names, name_bytes) != I2I_OK) return fail("read");
    names[name_bytes] = 0;
    size_t n_bad = 0;
    for (size_t b = 0; b < B; ++b) {
        const uint32_t* v = verdict + 4 * b;
        if (v[0] > n_taps || v[1] > n_taps) { fprintf(stderr, "batch_health_host: verdict row %zu names tap %u / %u of %zu\n", b, v[0], v[1], n_taps); return 1; }
        printf("request %zu: %s%s  first over the limit: %s  runs %u bad_runs %u\n", b, v[0] ? "first non-finite tensor: " : "finite",
               v[0] ? label_of(names, name_bytes, v[0] - 1) : "", v[1] ? label_of(names, name_bytes, v[1] - 1) : "none", v[2], v[3]);
        n_bad += v[0] != 0;
    }
    printf("batch_health_host: %zu of %zu requests non-finite in the last run (%zu taps, %s)\n", n_bad, B, n_taps, i2i_backend());
    free(verdict);
    free(names);
    i2i_plan_destroy(plan);
    return n_bad ? 3 : 0;
}
