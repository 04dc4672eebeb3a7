// Stand-alone host program for a sanitizer build: the size and refusal logic of tvr_density_volume_bytes / tvr_scene_set_density_volume (include/tvr.h), on the CPU.
// Nothing is launched: the scenes' parameters are never packed, so an accepted attach only records the pointer.  Build and run (scripts/sanitize/README.md):
//   make -C scripts/sanitize run
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../include/tvr.h"

static int failures = 0;
#define EXPECT(cond)                                                                          \
    do {                                                                                      \
        if (!(cond)) { ++failures; fprintf(stderr, "%s:%d: EXPECT(%s) failed — last error: %s\n", __FILE__, __LINE__, #cond, tvr_last_error()); } \
    } while (0)

static tvr_scene_desc make_desc(int gx, int gy, int gz, int n_sigma, int n_app)
{
    tvr_scene_desc d;
    memset(&d, 0, sizeof(d));
    const int g[3] = {gx, gy, gz};
    for (int k = 0; k < 3; ++k) {
        d.grid[k] = g[k];
        d.aabb[k] = -1.5f;
        d.aabb[3 + k] = 1.5f;
        d.inv_aabb_size[k] = 2.0f / 3.0f;
        d.density_n_comp[k] = n_sigma;
        d.app_n_comp[k] = n_app;
    }
    d.app_dim = 27; d.featureC = 128; d.view_pe = 2; d.fea_pe = 2;
    d.step_size = 0.005f;
    return d;
}

static void *aligned(void *p, size_t a) { return (void *)(((uintptr_t)p + a - 1) / a * a); }

int main()
{
    // sizes: cubic, non-cubic, the ABI's extremes, bad descriptors
    const int grids[][3] = {{300, 300, 300}, {5, 7, 9}, {2, 2, 2}, {4096, 4096, 4096}, {64, 3, 4096}};
    for (const auto &g : grids) {
        tvr_scene_desc d = make_desc(g[0], g[1], g[2], 16, 48);
        EXPECT(tvr_density_volume_bytes(&d) == 4ull * (size_t)(g[0] + 1) * (size_t)(g[1] + 1) * (size_t)(g[2] + 1));
    }
    { tvr_scene_desc d = make_desc(1, 300, 300, 16, 48); EXPECT(tvr_density_volume_bytes(&d) == 0); }
    { tvr_scene_desc d = make_desc(300, 300, 4097, 16, 48); EXPECT(tvr_density_volume_bytes(&d) == 0); }
    { tvr_scene_desc d = make_desc(300, 300, 300, 17, 48); EXPECT(tvr_density_volume_bytes(&d) == 0); }
    EXPECT(tvr_density_volume_bytes(nullptr) == 0);

    // refusals and attach / detach on a scene whose packed buffer is host memory that is never dereferenced
    tvr_scene_desc d = make_desc(5, 7, 9, 16, 48);
    const size_t need = tvr_density_volume_bytes(&d), packed = tvr_scene_packed_bytes(&d);
    EXPECT(need == 4u * 6 * 8 * 10 && packed > 0);
    char *pk_raw = (char *)malloc(512), *vol_raw = (char *)malloc(need + 512);
    void *pk = aligned(pk_raw, 256), *vol = aligned(vol_raw, 256);
    tvr_scene *s = nullptr;
    EXPECT(tvr_scene_create(&d, pk, packed, &s) == TVR_OK && s);
    EXPECT(tvr_scene_set_density_volume(nullptr, vol, need, nullptr) == TVR_ERR_INVALID);
    EXPECT(tvr_scene_set_density_volume(s, vol, need - 1, nullptr) == TVR_ERR_SCRATCH);
    EXPECT(tvr_scene_set_density_volume(s, vol, 0, nullptr) == TVR_ERR_SCRATCH);
    EXPECT(tvr_scene_set_density_volume(s, (char *)vol + 4, need + 128, nullptr) == TVR_ERR_SCRATCH);
    EXPECT(tvr_scene_set_density_volume(s, (char *)vol + 128, need + 128, nullptr) == TVR_ERR_SCRATCH);
    EXPECT(tvr_scene_set_density_volume(s, vol, need, nullptr) == TVR_OK);
    EXPECT(tvr_scene_set_density_volume(s, vol, need - 1, nullptr) == TVR_ERR_SCRATCH);      // a refused call leaves the attached volume alone
    EXPECT(tvr_scene_touch(s) == TVR_OK);
    EXPECT(tvr_scene_set_density_volume(s, nullptr, 0, nullptr) == TVR_OK);
    EXPECT(tvr_scene_set_density_volume(s, nullptr, 0, nullptr) == TVR_OK);
    EXPECT(tvr_scene_destroy(s) == TVR_OK);

    // a CP scene refuses a volume (and accepts a detach)
    tvr_scene_desc c = make_desc(5, 7, 9, 96, 288);
    const size_t cpk = tvr_cp_scene_packed_bytes(&c);
    tvr_scene *cs = nullptr;
    EXPECT(cpk > 0 && tvr_cp_scene_create(&c, pk, cpk, &cs) == TVR_OK && cs);
    EXPECT(tvr_scene_set_density_volume(cs, vol, need, nullptr) == TVR_ERR_UNSUPPORTED && strstr(tvr_last_error(), "CP"));
    EXPECT(tvr_scene_set_density_volume(cs, nullptr, 0, nullptr) == TVR_OK);
    EXPECT(tvr_scene_destroy(cs) == TVR_OK);
    free(pk_raw);
    free(vol_raw);
    printf(failures ? "density_volume_host: %d FAILURES\n" : "density_volume_host: ok\n", failures);
    return failures ? 1 : 0;
}
