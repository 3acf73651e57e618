/* A batching host that is not Python: B requests packed into one planned forward, each with its own seed.
 *
 *     python -m img2img_turbo_amd.plan_file --out bs3.i2iplan --batch 3 --seeds 0,0,0 ...        (a per-image plan: "seed" is 16 * B bytes)
 *     cc -O2 -I include examples/batch_host.c -o batch_host -L img2img-turbo_amd/csrc -li2i_turbo -Wl,-rpath,img2img-turbo_amd/csrc
 *     ./batch_host bs3.i2iplan x.bin ctx.bin eps_out.bin out.bin SEED0 SEED1 SEED2 [noise_out.bin]
 *
 * The plan draws its own noise from one state row per image (include/i2i_turbo.h, i2i_randn_batch_params: row b = {seed_lo, seed_hi, step,
 * reserved}), so the noise of a request is what a batch-1 run draws at its seed, whatever slot it got.  The host writes the rows at step 0,
 * runs, and reads back "eps" (the noise the program drew; "noise" too with a sixth file name on a stochastic plan) and "out".  x.bin /
 * ctx.bin are the raw boundary buffers, as in examples/plan_host.c.  tests/test_batch_emu.py builds this file with gcc against the CPU
 * emulator library and checks both outputs against the Python replay bit for bit. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "i2i_turbo.h"

static int fail(const char* what) {
    fprintf(stderr, "batch_host: %s: %s\n", what, i2i_last_error());
    return 1;
}

static int feed(void* plan, const char* name, const char* path) {
    void* dev;
    size_t bytes;
    if (i2i_plan_io(plan, name, &dev, &bytes) != I2I_OK) return fail(name);
    void* host = malloc(bytes);
    FILE* f = fopen(path, "rb");
    if (!host || !f || fread(host, 1, bytes, f) != bytes) { fprintf(stderr, "batch_host: %s: cannot read %zu bytes from %s\n", name, bytes, path); return 1; }
    fclose(f);
    const int rc = i2i_plan_write(plan, name, host, bytes);
    free(host);
    return rc == I2I_OK ? 0 : fail(name);
}

static int fetch(void* plan, const char* name, const char* path, size_t* bytes_out) {
    void* dev;
    size_t bytes;
    if (i2i_plan_io(plan, name, &dev, &bytes) != I2I_OK) return fail(name);
    void* host = malloc(bytes);
    if (!host || i2i_plan_read(plan, name, host, bytes) != I2I_OK) return fail(name);
    FILE* f = fopen(path, "wb");
    if (!f || fwrite(host, 1, bytes, f) != bytes) { fprintf(stderr, "batch_host: cannot write %s\n", path); return 1; }
    fclose(f);
    free(host);
    if (bytes_out) *bytes_out = bytes;
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 7) { fprintf(stderr, "usage: %s plan x.bin ctx.bin eps_out.bin out.bin SEED0 [SEED1 ..] [noise_out.bin]\n", argv[0]); return 2; }
    if (i2i_abi_version() != I2I_ABI_VERSION) { fprintf(stderr, "batch_host: header / library ABI mismatch\n"); return 2; }
    void* plan = NULL;
    if (i2i_plan_load(argv[1], &plan) != I2I_OK) return fail("load");
    /* the seeds: every argument from the sixth on that parses as an integer; one more, if any, names the file for "noise" */
    uint64_t seeds[256];
    int n_seeds = 0, a = 6;
    for (; a < argc && n_seeds < 256; ++a) {
        char* end;
        const unsigned long long v = strtoull(argv[a], &end, 0);
        if (end == argv[a] || *end) break;
        seeds[n_seeds++] = (uint64_t)v;
    }
    const char* noise_path = a < argc ? argv[a] : NULL;
    void* dev;
    size_t seed_bytes;
    if (i2i_plan_io(plan, "seed", &dev, &seed_bytes) != I2I_OK) {
        fprintf(stderr, "batch_host: %s has no \"seed\" buffer: export it with --seeds (one noise state per image)\n", argv[1]);
        return 1;
    }
    if (seed_bytes != 16u * (size_t)n_seeds) {
        fprintf(stderr, "batch_host: \"seed\" holds %zu bytes but %d seeds x 16 = %zu were given: a per-image plan (--seeds) has one 16-byte row "
                        "per image, a plan exported with --seed has 16 bytes for the whole batch\n", seed_bytes, n_seeds, 16u * (size_t)n_seeds);
        return 1;
    }
    uint32_t states[256][4];
    for (int b = 0; b < n_seeds; ++b) {
        states[b][0] = (uint32_t)seeds[b];
        states[b][1] = (uint32_t)(seeds[b] >> 32);
        states[b][2] = 0;      /* step: every run adds one */
        states[b][3] = 0;      /* reserved */
    }
    if (i2i_plan_write(plan, "seed", states, seed_bytes) != I2I_OK) return fail("seed");
    if (feed(plan, "x", argv[2]) || feed(plan, "ctx", argv[3])) return 1;
    if (i2i_plan_run(plan, NULL) != I2I_OK) return fail("run");      /* NULL = the default stream */
    size_t out_bytes = 0;
    if (fetch(plan, "eps", argv[4], NULL) || fetch(plan, "out", argv[5], &out_bytes)) return 1;
    if (noise_path && fetch(plan, "noise", noise_path, NULL)) return 1;
    i2i_plan_destroy(plan);
    printf("batch_host: %s on %s, %d images, %zu output bytes\n", argv[1], i2i_backend(), n_seeds, out_bytes);
    return 0;
}
