/* A host that is not Python on an automatic-threshold edge plan: photos in, thresholds chosen by the program, edge map and image out.
 *
 *     python -m img2img_turbo_amd.plan_file --out edge.i2iplan --u8 --canny-auto 0.33 ...        ("x" holds photos; the program starts with
 *                                                                                                  i2i_canny_auto_thr, then Canny)
 *     cc -O2 -I include examples/auto_canny_host.c -o auto_canny_host -L img2img-turbo_amd/csrc -li2i_turbo -Wl,-rpath,img2img-turbo_amd/csrc
 *     ./auto_canny_host edge.i2iplan x.bin ctx.bin eps.bin thr_out.bin edges_out.bin out.bin [SIGMA]
 *
 * The thresholds are device state the program WRITES (include/i2i_turbo.h, i2i_canny_auto_thr_params: the median rule per image, low =
 * (1 - sigma) * median, high = (1 + sigma) * median in integers), so nothing is downloaded, chosen on the host and uploaded between the
 * photo and the generator.  "canny_sigma" holds sigma * 65536 per image as saved at export; with SIGMA the host overwrites every entry (a
 * negative entry would make that image keep the pair written to "canny_thr").  After the run "canny_thr" holds the {low, high} pairs that
 * were used, "canny_edges" the edge map the generator saw (255 on edges) and "out" the image.  x.bin / ctx.bin / eps.bin are the raw
 * boundary buffers, as in examples/plan_host.c.  tests/test_canny_auto_emu.py builds this file with gcc against the CPU emulator library
 * and checks the three outputs against the Python run bit for bit. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "i2i_turbo.h"

static int fail(const char* what) {
    fprintf(stderr, "auto_canny_host: %s: %s\n", what, i2i_last_error());
    return 1;
}

static int feed(void* plan, const char* name, const char* path) {
    void* dev;
    size_t bytes;
    if (i2i_plan_io(plan, name, &dev, &bytes) != I2I_OK) return fail(name);
    void* host = malloc(bytes);
    FILE* f = fopen(path, "rb");
    if (!host || !f || fread(host, 1, bytes, f) != bytes) { fprintf(stderr, "auto_canny_host: %s: cannot read %zu bytes from %s\n", name, bytes, path); return 1; }
    fclose(f);
    const int rc = i2i_plan_write(plan, name, host, bytes);
    free(host);
    return rc == I2I_OK ? 0 : fail(name);
}

static int fetch(void* plan, const char* name, const char* path, void** keep, size_t* bytes_out) {
    void* dev;
    size_t bytes;
    if (i2i_plan_io(plan, name, &dev, &bytes) != I2I_OK) return fail(name);
    void* host = malloc(bytes);
    if (!host || i2i_plan_read(plan, name, host, bytes) != I2I_OK) return fail(name);
    FILE* f = fopen(path, "wb");
    if (!f || fwrite(host, 1, bytes, f) != bytes) { fprintf(stderr, "auto_canny_host: cannot write %s\n", path); return 1; }
    fclose(f);
    if (keep) *keep = host;
    else free(host);
    if (bytes_out) *bytes_out = bytes;
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 8) { fprintf(stderr, "usage: %s plan x.bin ctx.bin eps.bin thr_out.bin edges_out.bin out.bin [SIGMA]\n", argv[0]); return 2; }
    if (i2i_abi_version() != I2I_ABI_VERSION) { fprintf(stderr, "auto_canny_host: header / library ABI mismatch\n"); return 2; }
    void* plan = NULL;
    if (i2i_plan_load(argv[1], &plan) != I2I_OK) return fail("load");
    void* dev;
    size_t sigma_bytes;
    if (i2i_plan_io(plan, "canny_sigma", &dev, &sigma_bytes) != I2I_OK) {
        fprintf(stderr, "auto_canny_host: %s has no \"canny_sigma\" buffer: export it with --canny-auto SIGMA\n", argv[1]);
        return 1;
    }
    const int images = (int)(sigma_bytes / 4);
    if (argc > 8) {                                          /* one sigma for every image of this run */
        const double sigma = atof(argv[8]);
        if (!(sigma >= 0.0 && sigma <= 1.0)) { fprintf(stderr, "auto_canny_host: SIGMA must lie in 0 .. 1\n"); return 2; }
        int32_t* q = (int32_t*)malloc(sigma_bytes);
        if (!q) return 1;
        for (int b = 0; b < images; ++b) q[b] = (int32_t)(sigma * 65536.0 + 0.5);
        const int rc = i2i_plan_write(plan, "canny_sigma", q, sigma_bytes);
        free(q);
        if (rc != I2I_OK) return fail("canny_sigma");
    }
    if (feed(plan, "x", argv[2]) || feed(plan, "ctx", argv[3]) || feed(plan, "eps", argv[4])) return 1;
    if (i2i_plan_run(plan, NULL) != I2I_OK) return fail("run");      /* NULL = the default stream */
    void* thr = NULL;
    size_t thr_bytes = 0, out_bytes = 0;
    if (fetch(plan, "canny_thr", argv[5], &thr, &thr_bytes) || fetch(plan, "canny_edges", argv[6], NULL, NULL) || fetch(plan, "out", argv[7], NULL, &out_bytes))
        return 1;
    uint32_t* med = (uint32_t*)malloc(sigma_bytes);
    if (!med || i2i_plan_read(plan, "canny_median2", med, sigma_bytes) != I2I_OK) return fail("canny_median2");
    for (int b = 0; b < images && (size_t)b * 8 < thr_bytes; ++b)
        printf("auto_canny_host: image %d: median %.1f -> low %d, high %d\n", b, med[b] / 2.0, ((int32_t*)thr)[2 * b], ((int32_t*)thr)[2 * b + 1]);
    free(med);
    free(thr);
    i2i_plan_destroy(plan);
    printf("auto_canny_host: %s on %s, %d images, %zu output bytes\n", argv[1], i2i_backend(), images, out_bytes);
    return 0;
}
