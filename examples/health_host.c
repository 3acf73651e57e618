/* Numerical health of a planned forward from a host that is not Python: loads a plan file exported with health scans
 * (python -m img2img_turbo_amd.plan_file --health stages|all ...), runs it, and prints one line per scanned tensor.
 *
 *     cc -O2 -I include examples/health_host.c -o health_host -L img2img-turbo_amd/csrc -li2i_turbo -Wl,-rpath,img2img-turbo_amd/csrc
 *     ./health_host pix2pix_bs8_512_health.i2iplan x.bin ctx.bin eps.bin [runs]
 *
 * "health" holds 8 uint64 per scanned tensor, in program order (include/i2i_turbo.h, i2i_scan_params: runs, NaN, +Inf, -Inf, finite values
 * over the limit, the fp32 bits of the largest finite |x|, elements, reserved), accumulated over the runs; "health_names" holds their
 * labels, each NUL-terminated.  Exit status: 0 = every tensor finite, 3 = some tensor held a NaN or an Inf (the first one is named),
 * 1 / 2 = errors.  tests/test_health_emu.py builds this file with gcc against the CPU emulator library. */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "i2i_turbo.h"

static int fail(const char* what) {
    fprintf(stderr, "health_host: %s: %s\n", what, i2i_last_error());
    return 1;
}

static int feed(void* plan, const char* name, const char* path) {
    void* dev;
    size_t bytes;
    if (i2i_plan_io(plan, name, &dev, &bytes) != I2I_OK) return fail(name);
    void* host = malloc(bytes);
    FILE* f = fopen(path, "rb");
    if (!host || !f || fread(host, 1, bytes, f) != bytes) { fprintf(stderr, "health_host: %s: cannot read %zu bytes from %s\n", name, bytes, path); return 1; }
    fclose(f);
    const int rc = i2i_plan_write(plan, name, host, bytes);
    free(host);
    return rc == I2I_OK ? 0 : fail(name);
}

int main(int argc, char** argv) {
    if (argc < 5) { fprintf(stderr, "usage: %s plan x.bin ctx.bin eps.bin [runs]\n", argv[0]); return 2; }
    if (i2i_abi_version() != I2I_ABI_VERSION) { fprintf(stderr, "health_host: header / library ABI mismatch\n"); return 2; }
    const int runs = argc > 5 ? atoi(argv[5]) : 1;
    void* plan = NULL;
    if (i2i_plan_load(argv[1], &plan) != I2I_OK) return fail("load");
    void* dev;
    size_t rec_bytes, name_bytes;
    if (i2i_plan_io(plan, "health", &dev, &rec_bytes) != I2I_OK || i2i_plan_io(plan, "health_names", &dev, &name_bytes) != I2I_OK) {
        fprintf(stderr, "health_host: %s carries no health scans (export it with --health)\n", argv[1]);
        return 2;
    }
    if (feed(plan, "x", argv[2]) || feed(plan, "ctx", argv[3]) || feed(plan, "eps", argv[4])) return 1;
    for (int i = 0; i < runs; ++i)
        if (i2i_plan_run(plan, NULL) != I2I_OK) return fail("run");
    uint64_t* rec = (uint64_t*)malloc(rec_bytes);
    char* names = (char*)malloc(name_bytes + 1);
    if (!rec || !names) return 1;
    if (i2i_plan_read(plan, "health", rec, rec_bytes) != I2I_OK || i2i_plan_read(plan, "health_names", names, name_bytes) != I2I_OK) return fail("read");
    names[name_bytes] = 0;
    const size_t n_taps = rec_bytes / 64;
    const char* label = names;
    const char* first_bad = NULL;
    for (size_t t = 0; t < n_taps; ++t) {
        const uint64_t* r = rec + 8 * t;
        const uint32_t bits = (uint32_t)r[5];
        float max_abs;
        memcpy(&max_abs, &bits, sizeof(max_abs));
        const int bad = r[1] || r[2] || r[3];
        printf("%-56s runs %" PRIu64 " nan %" PRIu64 " +inf %" PRIu64 " -inf %" PRIu64 " over %" PRIu64 " max_abs %.6g elements %" PRIu64 "%s\n",
               label, r[0], r[1], r[2], r[3], r[4], (double)max_abs, r[6], bad ? "  <-- non-finite" : "");
        if (bad && !first_bad) first_bad = label;
        if (label < names + name_bytes) label += strlen(label) + 1;
    }
    int status = 0;
    if (first_bad) {
        printf("health_host: first non-finite tensor: %s\n", first_bad);
        status = 3;
    } else {
        printf("health_host: %zu tensors, all finite (%s)\n", n_taps, i2i_backend());
    }
    free(rec);
    free(names);
    i2i_plan_destroy(plan);
    return status;
}
