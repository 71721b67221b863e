// capi_walls.inc — domain walls: the launch enqueue_finish puts between the grid update and the fused G2P on data that has walls
// set (launch_grid_walls, declared in host_substep.inc), and the two entry points. The kernel is in kernels_walls.h. The walls live
// in the handle (wgs_data::walls) and travel as a kernel argument: no device memory, no upload, nothing in Dev.

namespace {

void launch_grid_walls(wgs_data *d) {
    static_assert(sizeof(WallSet) == 72 && sizeof(wgs_wall) == 12, "the walls are a 72-byte kernel argument in both dimensions");
    WallSet w{};
    for (int f = 0; f < 2 * D; f++) {
        w.type[f] = d->walls[f].type;
        w.friction[f] = d->walls[f].friction;
        w.plane[f] = d->walls[f].plane;
    }
    // one wave per active block as the host last saw them (the waves stride over whatever the list holds now)
    const uint32_t blocks = d->seen.nblocks ? d->seen.nblocks : d->dev.cap;
    const uint32_t wgs_n = std::max(64u, std::min((uint32_t)grid_for(d, WGS_GU_WG_PER_CU), (blocks + 3u) / 4u));
    hipLaunchKernelGGL(k_grid_walls<D>, dim3(wgs_n), dim3(256), 0, d->stream, d->dev, w);
}

}  // namespace

extern "C" {

wgs_status wgs_set_domain_walls(wgs_data *d, const wgs_wall *walls) {
    WGS_TRY(enter(d));
    if (d->dev.sharded) return fail(WGS_ERR_UNSUPPORTED, "wgs_set_domain_walls: sharded wgs_data (a slab holds a part of the grid): single-domain data only");
    bool any = false;
    if (walls) {
        for (int f = 0; f < 2 * D; f++) {
            if (walls[f].type > WGS_WALL_SEPARATE) return fail(WGS_ERR_INVALID_ARGUMENT, "wgs_set_domain_walls: wall type must be WGS_WALL_NONE .. WGS_WALL_SEPARATE");
            if (!std::isfinite(walls[f].friction) || walls[f].friction < 0.f) return fail(WGS_ERR_INVALID_ARGUMENT, "wgs_set_domain_walls: friction must be finite and >= 0");
            any |= walls[f].type != WGS_WALL_NONE;
        }
        for (int k = 0; k < D; k++)
            if (walls[2 * k].type != WGS_WALL_NONE && walls[2 * k + 1].type != WGS_WALL_NONE && walls[2 * k].plane >= walls[2 * k + 1].plane)
                return fail(WGS_ERR_INVALID_ARGUMENT, "wgs_set_domain_walls: the low plane of an axis must lie below its high plane");
    }
    for (int f = 0; f < 2 * D; f++) d->walls[f] = walls ? walls[f] : wgs_wall{WGS_WALL_NONE, 0.f, 0};
    d->walls_set = any;
    return WGS_OK;
}

wgs_status wgs_get_domain_walls(wgs_data *d, wgs_wall *out) {
    WGS_TRY(enter(d, out != nullptr));
    if (d->dev.sharded) return fail(WGS_ERR_UNSUPPORTED, "wgs_get_domain_walls: sharded wgs_data (a slab holds a part of the grid): single-domain data only");
    for (int f = 0; f < 2 * D; f++) out[f] = d->walls[f];
    return WGS_OK;
}

}  // extern "C"
