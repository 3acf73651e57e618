/* Device fingerprints from a host that is not Python: loads a plan file exported with fingerprints
 * (python -m img2img_turbo_amd.plan_file --fingerprint io|stages|all [--digests] ...), checks the file's own digests where it has them,
 * runs it, and prints one line per tap and image.
 *
 *     cc -O2 -I include examples/fingerprint_host.c -o fingerprint_host -L img2img-turbo_amd/csrc -li2i_turbo -Wl,-rpath,img2img-turbo_amd/csrc
 *     ./fingerprint_host pix2pix_bs8_512_fp.i2iplan x.bin ctx.bin eps.bin [--twice]
 *
 * "fingerprint" holds 4 uint64 per tap and image, tap-major (include/i2i_turbo.h, i2i_digest_params: s0, s1, elements, reserved), zeroed by
 * the program itself at the start of every run; "fingerprint_names" holds the tap labels, each NUL-terminated.  Two runs, two GPUs or two
 * hosts that computed the same bits print the same lines: diff them.  A file exported with --digests is verified first
 * (i2i_plan_verify: the weights, constants and tables as they sit in device memory against the records stored at export).
 * --twice runs the program a second time on the same inputs and compares every record (use a plan exported WITHOUT --seed: a seeded
 * plan advances its step and draws other noise).
 * Exit status: 0 = fine, 4 = the file's digests do not match (the buffer is named), 3 = the second run differs from the first (the first
 * differing tap and image are named), 1 / 2 = errors.  tests/test_digest_emu.py builds this file with gcc against the CPU emulator library. */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "i2i_turbo.h"

static int fail(const char* what) {
    fprintf(stderr, "fingerprint_host: %s: %s\n", what, i2i_last_error());
    return 1;
}

static int feed(void* plan, const char* name, const char* path) {
    void* dev;
    size_t bytes;
    if (i2i_plan_io(plan, name, &dev, &bytes) != I2I_OK) return fail(name);
    void* host = malloc(bytes);
    FILE* f = fopen(path, "rb");
    if (!host || !f || fread(host, 1, bytes, f) != bytes) { fprintf(stderr, "fingerprint_host: %s: cannot read %zu bytes from %s\n", name, bytes, path); return 1; }
    fclose(f);
    const int rc = i2i_plan_write(plan, name, host, bytes);
    free(host);
    return rc == I2I_OK ? 0 : fail(name);
}

int main(int argc, char** argv) {
    if (argc < 5) { fprintf(stderr, "usage: %s plan x.bin ctx.bin eps.bin [--twice]\n", argv[0]); return 2; }
    if (i2i_abi_version() != I2I_ABI_VERSION) { fprintf(stderr, "fingerprint_host: header / library ABI mismatch\n"); return 2; }
    const int twice = argc > 5 && strcmp(argv[5], "--twice") == 0;
    void* plan = NULL;
    if (i2i_plan_load(argv[1], &plan) != I2I_OK) return fail("load");
    int bad_buffer = -1;
    const int vrc = i2i_plan_verify(plan, NULL, &bad_buffer);
    if (vrc == I2I_ERR_MISMATCH) {
        fprintf(stderr, "fingerprint_host: %s is damaged (buffer %d): %s\n", argv[1], bad_buffer, i2i_last_error());
        return 4;
    }
    if (vrc != I2I_OK && vrc != I2I_ERR_UNSUPPORTED) return fail("verify");
    printf("fingerprint_host: %s\n", vrc == I2I_OK ? "weights verified against the file's digests" : "the file carries no digests (export it with --digests)");
    void* dev;
    size_t rec_bytes, name_bytes, x_bytes;
    if (i2i_plan_io(plan, "fingerprint", &dev, &rec_bytes) != I2I_OK || i2i_plan_io(plan, "fingerprint_names", &dev, &name_bytes) != I2I_OK) {
        fprintf(stderr, "fingerprint_host: %s carries no fingerprints (export it with --fingerprint io|stages|all)\n", argv[1]);
        return 2;
    }
    if (i2i_plan_io(plan, "x", &dev, &x_bytes) != I2I_OK) return fail("x");
    if (feed(plan, "x", argv[2]) || feed(plan, "ctx", argv[3]) || feed(plan, "eps", argv[4])) return 1;
    uint64_t* rec = (uint64_t*)malloc(rec_bytes);
    uint64_t* again = (uint64_t*)malloc(rec_bytes);
    char* names = (char*)malloc(name_bytes + 1);
    if (!rec || !again || !names) return 1;
    if (i2i_plan_run(plan, NULL) != I2I_OK) return fail("run");
    if (i2i_plan_read(plan, "fingerprint", rec, rec_bytes) != I2I_OK || i2i_plan_read(plan, "fingerprint_names", names, name_bytes) != I2I_OK) return fail("read");
    names[name_bytes] = 0;
    size_t n_taps = 0;
    for (size_t i = 0; i < name_bytes; ++i) n_taps += names[i] == 0;
    if (n_taps == 0 || rec_bytes % (32 * n_taps)) { fprintf(stderr, "fingerprint_host: %zu labels for %zu bytes of records\n", n_taps, rec_bytes); return 1; }
    const size_t images = rec_bytes / (32 * n_taps);
    const char* label = names;
    for (size_t t = 0; t < n_taps; ++t) {
        for (size_t b = 0; b < images; ++b) {
            const uint64_t* r = rec + 4 * (t * images + b);
            printf("tap %s image %zu: %016" PRIx64 " %016" PRIx64 " elements %" PRIu64 "\n", label, b, r[0], r[1], r[2]);
        }
        label += strlen(label) + 1;
    }
    int status = 0;
    if (twice) {
        if (i2i_plan_run(plan, NULL) != I2I_OK) return fail("second run");
        if (i2i_plan_read(plan, "fingerprint", again, rec_bytes) != I2I_OK) return fail("read");
        label = names;
        for (size_t t = 0; t < n_taps && !status; ++t) {
            for (size_t b = 0; b < images && !status; ++b) {
                if (memcmp(rec + 4 * (t * images + b), again + 4 * (t * images + b), 32) != 0) {
                    printf("fingerprint_host: the second run differs from the first at tap %s image %zu\n", label, b);
                    status = 3;
                }
            }
            label += strlen(label) + 1;
        }
        if (!status) printf("fingerprint_host: two runs, %zu taps x %zu images, bit-identical (%s)\n", n_taps, images, i2i_backend());
    }
    free(rec);
    free(again);
    free(names);
    i2i_plan_destroy(plan);
    return status;
}
