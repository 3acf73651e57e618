/* The LoRA scale slider of gradio_sketch2image.py:67-91 in a host that is not Python: loads a plan file exported with live_scale
 * (img2img_turbo_amd.plan_file.export_plan(plan, path, live_scale=True), or `plan_file --live-scale`) and runs the forward once per
 * scale r given on the command line, moving r with i2i_plan_set_scale() -- a few bytes of device state and the scale program, no new
 * file, no upload of weights.
 *
 *     cc -O2 -I include examples/slider_host.c -o slider_host -L img2img-turbo_amd/csrc -li2i_turbo -Wl,-rpath,img2img-turbo_amd/csrc
 *     ./slider_host sketch_bs1_512.i2iplan x.bin ctx.bin eps.bin noise.bin out 0.4 1.0        -> out_0.bin (r = 0.4), out_1.bin (r = 1.0)
 *
 * The .bin files are the raw contents of the boundary buffers, as for examples/plan_host.c; pass "-" for noise.bin on a plan without a
 * noise map.  The skip gamma follows r, as the reference sets both (src/pix2pix_turbo.py:206-217). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "i2i_turbo.h"

static int fail(const char* what) {
    fprintf(stderr, "slider_host: %s: %s\n", what, i2i_last_error());
    return 1;
}

static int feed(void* plan, const char* name, const char* path) {
    void* dev;
    size_t bytes;
    if (i2i_plan_io(plan, name, &dev, &bytes) != I2I_OK) return fail(name);
    void* host = malloc(bytes);
    FILE* f = fopen(path, "rb");
    if (!host || !f || fread(host, 1, bytes, f) != bytes) { fprintf(stderr, "slider_host: %s: cannot read %zu bytes from %s\n", name, bytes, path); return 1; }
    fclose(f);
    const int rc = i2i_plan_write(plan, name, host, bytes);
    free(host);
    return rc == I2I_OK ? 0 : fail(name);
}

int main(int argc, char** argv) {
    if (argc < 8) { fprintf(stderr, "usage: %s plan x.bin ctx.bin eps.bin noise.bin|- out_prefix r [r ...]\n", argv[0]); return 2; }
    if (i2i_abi_version() != I2I_ABI_VERSION) { fprintf(stderr, "slider_host: header / library ABI mismatch\n"); return 2; }
    void* plan = NULL;
    if (i2i_plan_load(argv[1], &plan) != I2I_OK) return fail("load");
    if (!i2i_plan_has_scale(plan)) { fprintf(stderr, "slider_host: %s carries no scale program: export it with live_scale\n", argv[1]); return 2; }
    if (feed(plan, "x", argv[2]) || feed(plan, "ctx", argv[3]) || feed(plan, "eps", argv[4])) return 1;
    if (strcmp(argv[5], "-") != 0 && feed(plan, "noise", argv[5])) return 1;
    void* dev;
    size_t bytes;
    if (i2i_plan_io(plan, "out", &dev, &bytes) != I2I_OK) return fail("out");
    void* host = malloc(bytes);
    if (!host) return 1;
    for (int i = 7; i < argc; ++i) {
        const float r = (float)atof(argv[i]);
        /* both calls only enqueue on the stream (NULL = the default one): the forward sees the weights the scale program wrote */
        if (i2i_plan_set_scale(plan, r, r, NULL) != I2I_OK) return fail("set_scale");
        if (i2i_plan_run(plan, NULL) != I2I_OK) return fail("run");
        if (i2i_plan_read(plan, "out", host, bytes) != I2I_OK) return fail("read");
        char path[1024];
        snprintf(path, sizeof(path), "%s_%d.bin", argv[6], i - 7);
        FILE* f = fopen(path, "wb");
        if (!f || fwrite(host, 1, bytes, f) != bytes) { fprintf(stderr, "slider_host: cannot write %s\n", path); return 1; }
        fclose(f);
        printf("slider_host: r = %g -> %s (%zu bytes)\n", (double)r, path, bytes);
    }
    free(host);
    i2i_plan_destroy(plan);
    return 0;
}
