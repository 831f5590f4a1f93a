// pt_rays_any.inc -- the any-hit loop of the ray queries, ONE text for two translation units: pt_kernels_rays.hip includes it where the function
// stood (k_traceRays, k_ao and k_viewAo call it) and keeps its kernels token for token; pt_kernels_view_batch.hip includes it for k_viewAoBatch.
// The includer has pt_rays_guard.hpp and is inside namespace pt.
// the per-set loop of the fused pass's shadow stage (pt_direct.hpp direct_all) on the caller's ray: the second statement of that loop,
// to be kept in step with the first by hand (see the header of pt_kernels_rays.hip)
template <bool FAST, int GRIDS>
PT_DEV void rays_any(const FusedArgs& A, Ray& sh, bool& defer) {
    if (FAST) guard_or_retire(sh, defer);
    const RayRcp rr = ray_rcp<FAST>(sh);
    for (uint32_t s = 0; s < A.n_sets; ++s) {
        const GridArgs& S = A.sets[s];
        keep_in_loop(sh);
        const bool live = !(sh.mint == sh.maxt);
        Hit ch;
        ch.idx = UINT32_MAX;
        ch.t = sh.maxt;
        bool walked = false;
        if (!GRIDS || S.n == 1u) {
            if (live) {
                const BoxHit bh = cell1_box<FAST>(sh, rr, S);
                if (bh.v) {
                    ch = (S.kind == KIND_SPHERES) ? trace_cell1<SPHERES, true, TRI_A10, FAST, true>(sh, rr, bh, S) : trace_cell1<TRIANGLES, true, TRI_A10, FAST, true, PT_LANE_LISTS_FOR(FAST, GRIDS)>(sh, rr, bh, S);
                    walked = true;
                }
            }
        } else if (S.kind == KIND_TRIANGLES) {
            BoxHit bh = {};
            if (live) bh = inter_aabb_t<FAST, true>(sh, rr, set_box(S));
            walked = live && bh.v;
            ch = trace_dda_coop<COOP_ANY, FAST, GRIDS == 1>(walked, sh, rr, bh, S, defer);
        } else if (live) {
            const BoxHit bh = inter_aabb_t<FAST, true>(sh, rr, set_box(S));
            if (bh.v) {
                ch = trace_dda<SPHERES, true, TRI_A10, FAST, GRIDS == 1>(sh, bh, S, defer);
                walked = true;
            }
        }
        if (!walked) continue;
        sh.maxt = ch.t;
        if (ch.idx != UINT32_MAX) sh.mint = ch.t;
    }
}
