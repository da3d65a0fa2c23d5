// Columns of a batch: sosrt_set_columns / sosrt_set_columns_zones (zone tables, row lists, column groups of the order loop),
// the combined-matrix (mix) groups of their slab rows, and which aerosol / atmosphere phase set a column reads.  Host code.
#include <hip/hip_runtime.h>

#include <vector>

#include "handle.hpp"

using namespace sosrt;

// Combined-matrix groups of the current columns: the distinct (atmosphere set, aerosol set, ca, cr) of their aerosol zones
// (spec:321: (w_atm/4) f_atm on W_atm, (w_aer/4) f_aer on W_aer), per (column, slab).
struct MixGroups {
    std::vector<double> ca, cr;
    std::vector<int> set, gid /*[B][kMaxZones], -1: clear zone*/, gcol /*[B]: the live-column tilings, one slab per column*/;
    std::vector<int> atm;                // atmosphere set of a group (sosrt_set_atmosphere_sets; all 0 otherwise)
};
// groups the cache may hold: kMaxMixGroups while every column uses set 0 (what it always held), more with several sets in use
namespace sosrt {
int mix_group_cap(const sosrt_handle* h, bool sets) {
    if (h->cols.mix_groups_max < sosrt_handle::Columns::kMaxMixGroups) return h->cols.mix_groups_max < 0 ? 0 : h->cols.mix_groups_max;
    if (!sets) return sosrt_handle::Columns::kMaxMixGroups;
    const size_t per = (size_t)h->g.Dp * h->g.Wld * sizeof(double);
    size_t n = per ? sosrt_handle::Columns::kMixCacheBytes / per : 0;
    if (n > (size_t)sosrt_handle::Columns::kMaxMixGroupsSets) n = sosrt_handle::Columns::kMaxMixGroupsSets;
    if (n < (size_t)sosrt_handle::Columns::kMaxMixGroups) n = sosrt_handle::Columns::kMaxMixGroups;
    if (n > (size_t)h->cols.mix_groups_max) n = h->cols.mix_groups_max;
    return (int)n;
}
}  // namespace sosrt
// false: more than `cap` groups
static bool collect_mix_groups(const sosrt_handle* h, int B, const std::vector<int>& zset, const std::vector<int>& aset, int cap,
                               MixGroups& mg) {
    mg.gid.assign((size_t)B * kMaxZones, -1);
    mg.gcol.assign(B, 0);
    for (int b = 0; b < B; ++b) {
        for (int z = 0; z < h->cols.c_nz[b]; ++z) {
            if (!h->cols.c_zmix[b * kMaxZones + z]) continue;
            const double da = h->cols.c_dtau_atm[b], dr = h->cols.c_zdtr[b * kMaxZones + z];
            const double ca = (h->cols.c_alb_atm[b] / 4) * (da / (da + dr)), cr = (h->cols.c_zwr[b * kMaxZones + z] / 4) * (dr / (da + dr));
            const int st = zset[b * kMaxZones + z], at = aset[b];
            int k = 0;
            while (k < (int)mg.ca.size() && !(mg.ca[k] == ca && mg.cr[k] == cr && mg.set[k] == st && mg.atm[k] == at)) ++k;
            if (k == (int)mg.ca.size()) {
                if (k == cap) return false;
                mg.ca.push_back(ca); mg.cr.push_back(cr); mg.set.push_back(st); mg.atm.push_back(at);
            }
            mg.gid[b * kMaxZones + z] = k;
            mg.gcol[b] = k;
        }
    }
    return true;
}
// uploads the groups and lists the slab rows of the dense contraction group by group.  A failed allocation of the cache leaves
// the two-pass form (mix_groups = 0) over the row lists as sosrt_set_columns wrote them -- a choice that is only open while
// every column uses set 0, so with sets in use it is an error.
static int apply_mix_groups(sosrt_handle* h, int B, const MixGroups& mg) {
    const int L = h->L;
    const std::vector<int>&nz = h->cols.c_nz, &zr0 = h->cols.c_zr0;
    auto zone_end = [&](int b, int z) { return z + 1 < nz[b] ? zr0[b * kMaxZones + z + 1] - 1 : L - 1; };
    const size_t per = (size_t)h->g.Dp * h->g.Wld, need = per * mg.ca.size();
    if (h->cols.d_Wmix.reserve(need)) {
        (void)hipGetLastError();
        if (h->cols.max_set_used > 0 || h->cols.max_atm_used > 0) {
            h->have_cols = false;
            return fail(SOSRT_E_NOMEM, "no memory for the %zu combined matrices of a batch with several phase sets", mg.ca.size());
        }
        return 0;
    }
    HIPCHK(hipMemcpy(h->cols.d_mixca, mg.ca.data(), mg.ca.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->cols.d_mixcr, mg.cr.data(), mg.cr.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->cols.d_mixset, mg.set.data(), mg.set.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->cols.d_mixatm, mg.atm.data(), mg.atm.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->cols.d_mixgroup, mg.gcol.data(), B * sizeof(int), hipMemcpyHostToDevice));
    h->cols.mix_groups = (int)mg.ca.size();
    // slab rows of the dense contraction listed, per column group of the order loop, group by group, every group padded
    // to whole 32-row tiles
    std::vector<int> grouped, tilegroup;
    for (int cg = 0; cg < h->grp.ngroups; ++cg) {
        for (int k = 0; k < h->cols.mix_groups; ++k) {
            for (int b = h->grp.gb[cg]; b < h->grp.gb[cg + 1]; ++b)
                for (int z = 0; z < nz[b]; ++z)
                    if (mg.gid[b * kMaxZones + z] == k)
                        for (int t = zr0[b * kMaxZones + z]; t <= zone_end(b, z); ++t) grouped.push_back(b * L + t);
            while (grouped.size() % 64) grouped.push_back(-1);   // whole 64-row tiles (two 32-row tiles of the same group)
            while (tilegroup.size() < grouped.size() / 32) tilegroup.push_back(k);
        }
        h->grp.slab_off[cg + 1] = (int)grouped.size();
    }
    HIPCHK(hipMemcpy(h->cols.d_slabrows, grouped.data(), grouped.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->cols.d_slabtilegroup, tilegroup.data(), tilegroup.size() * sizeof(int), hipMemcpyHostToDevice));
    h->cols.nslab = (int)grouped.size();
    h->cols.mix_dirty = true;
    h->phase.w32_dirty = true;
    return 0;
}

// Common part of sosrt_set_columns / sosrt_set_columns_zones: zone tables [B][kMaxZones] (host), per-column scalars.
static int set_columns_impl(sosrt_handle* h, int B, int geometry, int surface, const std::vector<int>& nz,
                            const std::vector<int>& zr0, const std::vector<int>& zmix, const std::vector<double>& zwr,
                            const std::vector<double>& zdtr, const double* mu0, const double* grd_alb, const double* alb_atm,
                            const double* dtau_atm, const double* tauStar_tot) {
    const size_t mb = h->max_batch;
    const int L = h->L;
    h->resident = false;                     // the descriptors of the resident field's columns are about to change
    h->cols.rw_on = false;                   // per-level weights belong to the columns they were set for
    h->cols.rw_regrouped = false;
    std::vector<double> sc(7 * mb, 0.0);
    std::vector<int> slab, plain, iup(B, 0), idn(B, 0);
    auto zone_end = [&](int b, int z) { return z + 1 < nz[b] ? zr0[b * kMaxZones + z + 1] - 1 : L - 1; };
    // column groups of the order loop: two contiguous halves for a large batch
    // (auto: two groups for a batch of more than SPLIT_MIN columns (48; 256 in round 3).  Round 3, EVA / wildfire sweeps with one and two groups
    // alternating on one box: 288 x (200, 128) 3.65 -> 3.33 ms, 320 x 3.89 -> 3.50, 512 x 5.03 -> 4.75, 1024 x 9.2 -> 8.15,
    // 2048 x 16.6 -> 15.5, 4096 x 32.4 -> 30.3; 512 x (200, 64) 3.02 -> 2.94, 1024 x (200, 64) 5.10 -> 4.69; 512 x (200, 256)
    // 13.1 -> 12.65, 512 x (400, 256) 13.5 -> 12.8, 4096 x (400, 256) 106 -> 103.7; 256 x (200, 128) unchanged.  The gain is the
    // MFMA-bound contraction of one half running beside the HBM-bound transport of the other; the HBM bytes of a solve are the same
    // either way: 17.6 vs 18.0 GB by PMC)
    int want = h->grp.want_groups;
    if (want == 0) want = B > h->grp.split_min ? 2 : 1;
    h->grp.ngroups = (want >= 2 && B >= h->grp.split_min && B >= 2) ? 2 : 1;
    if (h->grp.ngroups > 1 && !h->grp.stream2) {
        HIPCHK(hipSetDevice(h->device));
        if (h->grp.prio2) {
            int least = 0, greatest = 0;
            HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
            HIPCHK(hipStreamCreateWithPriority(&h->grp.stream2, hipStreamNonBlocking, h->grp.prio2 > 0 ? greatest : least));
        } else {
            HIPCHK(hipStreamCreateWithFlags(&h->grp.stream2, hipStreamNonBlocking));
        }
    }
    h->grp.gb[0] = 0; h->grp.gb[1] = h->grp.ngroups == 2 ? ((h->grp.split_at > 0 && h->grp.split_at < B) ? h->grp.split_at : B / 2) : B; h->grp.gb[2] = B;
    for (int k = 0; k <= sosrt_handle::kMaxGroups; ++k) { h->grp.main_off[k] = 0; h->grp.slab_off[k] = 0; }
    h->cols.max_nz = 1;
    h->cols.simple_zones = true;                  // every column is (clear, slab, clear): the live-column tilings apply
    if (geometry == SOSRT_GEOM_THREE_ZONE) {
        for (int b = 0; b < B; ++b) {
            h->cols.max_nz = nz[b] > h->cols.max_nz ? nz[b] : h->cols.max_nz;
            const int* m = &zmix[b * kMaxZones];
            if (!(nz[b] == 3 && m[0] == 0 && m[1] == 1 && m[2] == 0)) h->cols.simple_zones = false;
            if (nz[b] == 3) { iup[b] = zr0[b * kMaxZones + 1]; idn[b] = zr0[b * kMaxZones + 2] - 1; }
        }
        for (int k = 0; k < h->grp.ngroups; ++k) {
            for (int b = h->grp.gb[k]; b < h->grp.gb[k + 1]; ++b)
                for (int z = 0; z < nz[b]; ++z)
                    for (int t = zr0[b * kMaxZones + z]; t <= zone_end(b, z); ++t) (zmix[b * kMaxZones + z] ? slab : plain).push_back(b * L + t);
            h->grp.main_off[k + 1] = (int)plain.size();
            h->grp.slab_off[k + 1] = (int)slab.size();
        }
    }
    for (int b = 0; b < B; ++b) {
        if (!(mu0[b] > 0)) return fail(SOSRT_E_INVALID, "column %d: mu0 must be > 0", b);
        sc[0 * mb + b] = mu0[b];
        sc[1 * mb + b] = grd_alb ? grd_alb[b] : 0.0;
        sc[2 * mb + b] = alb_atm[b];
        sc[4 * mb + b] = dtau_atm ? dtau_atm[b] : 1.0;
        sc[6 * mb + b] = tauStar_tot[b];
    }
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(h->cols.d_scal, sc.data(), 7 * mb * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (geometry == SOSRT_GEOM_THREE_ZONE) {
        HIPCHK(hipMemcpyAsync(h->cols.d_nz, nz.data(), B * sizeof(int), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->cols.d_zr0, zr0.data(), (size_t)B * kMaxZones * sizeof(int), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->cols.d_zmix, zmix.data(), (size_t)B * kMaxZones * sizeof(int), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->cols.d_zwr, zwr.data(), (size_t)B * kMaxZones * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->cols.d_zdtr, zdtr.data(), (size_t)B * kMaxZones * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->cols.d_idx_up, iup.data(), B * sizeof(int), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->cols.d_idx_down, idn.data(), B * sizeof(int), hipMemcpyHostToDevice, h->stream));
        if (!slab.empty())
            HIPCHK(hipMemcpyAsync(h->cols.d_slabrows, slab.data(), slab.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
        if (!plain.empty())
            HIPCHK(hipMemcpyAsync(h->cols.d_mainrows, plain.data(), plain.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));   // the staging vectors go out of scope
    h->cols.nslab = (int)slab.size();
    h->cols.nmain = (int)plain.size();
    h->cols.max_main = L; h->cols.max_slab = 0;
    if (geometry == SOSRT_GEOM_THREE_ZONE) {
        h->cols.max_main = 0;
        for (int b = 0; b < B; ++b) {
            int ns = 0;
            for (int z = 0; z < nz[b]; ++z)
                if (zmix[b * kMaxZones + z]) ns += zone_end(b, z) - zr0[b * kMaxZones + z] + 1;
            h->cols.max_slab = ns > h->cols.max_slab ? ns : h->cols.max_slab;
            h->cols.max_main = L - ns > h->cols.max_main ? L - ns : h->cols.max_main;
        }
    }
    h->cols.mix_groups = 0;
    h->cols.mix_dirty = true;
    h->phase.w32_dirty = true;
    // every column starts on aerosol set 0 (sosrt_set_aerosol_sets changes that), P0_aer is one row per column
    h->cols.max_set_used = 0;
    h->cols.max_atm_used = 0;                     // ... and on atmosphere set 0 (sosrt_set_atmosphere_sets)
    h->cols.c_atmset.assign(B, 0);
    h->cols.p0_zones = 0;
    h->cols.c_nz = nz; h->cols.c_zr0 = zr0; h->cols.c_zmix = zmix; h->cols.c_zwr = zwr; h->cols.c_zdtr = zdtr;
    h->cols.c_zset.assign((size_t)B * kMaxZones, 0);
    h->cols.c_alb_atm.assign(alb_atm, alb_atm + B);
    h->cols.c_dtau_atm.assign(B, 1.0);
    if (dtau_atm) h->cols.c_dtau_atm.assign(dtau_atm, dtau_atm + B);
    if (geometry == SOSRT_GEOM_THREE_ZONE && h->cols.nslab > 0) {
        MixGroups mg;
        if (collect_mix_groups(h, B, h->cols.c_zset, h->cols.c_atmset, mix_group_cap(h, false), mg))
            if (int e = apply_mix_groups(h, B, mg)) return e;
    }
    h->B = B; h->geom = geometry; h->surface = surface;
    h->have_cols = true;
    return 0;
}

extern "C" {

int sosrt_set_columns(sosrt_t* h, int B, int geometry, int surface, const int* idx_up, const int* idx_down,
                      const double* mu0, const double* grd_alb, const double* alb_atm, const double* alb_aer,
                      const double* dtau_atm, const double* dtau_aer, const double* tauStar_tot) {
    if (int e = need_gpu(h)) return e;
    if (B < 1 || B > h->max_batch) return fail(SOSRT_E_INVALID, "B=%d outside 1..max_batch=%d", B, h->max_batch);
    if (!mu0 || !alb_atm || !tauStar_tot) return fail(SOSRT_E_INVALID, "mu0, alb_atm and tauStar_tot are required");
    std::vector<int> nz(B, 1), zr0((size_t)B * kMaxZones, 0), zmix((size_t)B * kMaxZones, 0);
    std::vector<double> zwr((size_t)B * kMaxZones, 0.0), zdtr((size_t)B * kMaxZones, 0.0);
    if (geometry == SOSRT_GEOM_THREE_ZONE) {
        if (!idx_up || !idx_down || !grd_alb || !alb_aer || !dtau_atm || !dtau_aer)
            return fail(SOSRT_E_INVALID, "three-zone geometry needs idx_up, idx_down, grd_alb, alb_aer, dtau_atm, dtau_aer");
        if (surface != SOSRT_SURFACE_SPECULAR && surface != SOSRT_SURFACE_LAMBERTIAN && surface != SOSRT_SURFACE_LAMBERTIAN_README)
            return fail(SOSRT_E_INVALID, "three-zone geometry needs a specular or lambertian surface");
        for (int b = 0; b < B; ++b) {
            if (idx_up[b] < 1 || idx_down[b] < idx_up[b] || idx_down[b] > h->L - 2)
                return fail(SOSRT_E_INVALID, "column %d: need 1 <= idx_up <= idx_down <= nb_layers-2 (got %d, %d)", b,
                            idx_up[b], idx_down[b]);
            // above / inside / below the aerosol slab (spec:113-449)
            nz[b] = 3;
            zr0[b * kMaxZones + 1] = idx_up[b]; zr0[b * kMaxZones + 2] = idx_down[b] + 1;
            zmix[b * kMaxZones + 1] = 1;
            zwr[b * kMaxZones + 1] = alb_aer[b];
            zdtr[b * kMaxZones + 1] = dtau_aer[b];
        }
    } else if (geometry == SOSRT_GEOM_SINGLE_SLAB) {
        surface = SOSRT_SURFACE_NONE;
    } else {
        return fail(SOSRT_E_INVALID, "unknown geometry %d", geometry);
    }
    return set_columns_impl(h, B, geometry, surface, nz, zr0, zmix, zwr, zdtr, mu0, grd_alb, alb_atm, dtau_atm, tauStar_tot);
}

int sosrt_set_columns_zones(sosrt_t* h, int B, int surface, int nzmax, const int* nz_in, const int* zone_r0, const int* zone_mix,
                            const double* mu0, const double* grd_alb, const double* alb_atm, const double* dtau_atm,
                            const double* zone_alb_aer, const double* zone_dtau_aer, const double* tauStar_tot) {
    if (int e = need_gpu(h)) return e;
    if (B < 1 || B > h->max_batch) return fail(SOSRT_E_INVALID, "B=%d outside 1..max_batch=%d", B, h->max_batch);
    if (!nz_in || !zone_r0 || !zone_mix || !mu0 || !grd_alb || !alb_atm || !dtau_atm || !zone_alb_aer || !zone_dtau_aer || !tauStar_tot)
        return fail(SOSRT_E_INVALID, "null argument");
    if (nzmax < 1 || nzmax > kMaxZones) return fail(SOSRT_E_INVALID, "nzmax must be in 1..%d (got %d)", kMaxZones, nzmax);
    if (surface != SOSRT_SURFACE_SPECULAR && surface != SOSRT_SURFACE_LAMBERTIAN && surface != SOSRT_SURFACE_LAMBERTIAN_README)
        return fail(SOSRT_E_INVALID, "a zone table needs a specular or lambertian surface");
    std::vector<int> nz(B), zr0((size_t)B * kMaxZones, 0), zmix((size_t)B * kMaxZones, 0);
    std::vector<double> zwr((size_t)B * kMaxZones, 0.0), zdtr((size_t)B * kMaxZones, 0.0);
    for (int b = 0; b < B; ++b) {
        nz[b] = nz_in[b];
        if (nz[b] < 1 || nz[b] > nzmax) return fail(SOSRT_E_INVALID, "column %d: %d zones, expected 1..%d", b, nz[b], nzmax);
        for (int z = 0; z < nz[b]; ++z) {
            const int r0 = zone_r0[b * nzmax + z], mix = zone_mix[b * nzmax + z] != 0;
            if (z == 0 ? r0 != 0 : !(r0 > zr0[b * kMaxZones + z - 1] && r0 < h->L))
                return fail(SOSRT_E_INVALID, "column %d: zone %d starts at row %d (zones start at 0 and ascend, below nb_layers)", b, z, r0);
            if (z > 0 && mix && zmix[b * kMaxZones + z - 1]) return fail(SOSRT_E_INVALID, "column %d: two adjacent aerosol zones (%d, %d): merge them", b, z - 1, z);
            // the reference's slab lies strictly inside the column (idx_up >= 1, idx_down <= L-2, spec:40): its formulas
            // read the rows either side of a slab
            if (mix && (z == 0 || z == nz[b] - 1)) return fail(SOSRT_E_INVALID, "column %d: an aerosol zone must have a clear zone above and below it", b);
            zr0[b * kMaxZones + z] = r0; zmix[b * kMaxZones + z] = mix;
            zwr[b * kMaxZones + z] = mix ? zone_alb_aer[b * nzmax + z] : 0.0;
            zdtr[b * kMaxZones + z] = mix ? zone_dtau_aer[b * nzmax + z] : 0.0;
            if (mix && !(zdtr[b * kMaxZones + z] >= 0)) return fail(SOSRT_E_INVALID, "column %d zone %d: dtau_aer must be >= 0", b, z);
        }
    }
    return set_columns_impl(h, B, SOSRT_GEOM_THREE_ZONE, surface, nz, zr0, zmix, zwr, zdtr, mu0, grd_alb, alb_atm, dtau_atm, tauStar_tot);
}

}  // extern "C"

// The slab rows of a batch with more groups than the cache, for the two passes (W_atm, then W_aer).  Every column on set 0:
// column by column, as sosrt_set_columns lists them.  With sets in use: per column group of the order loop set by set, every
// set padded to whole 64-row tiles, so that a tile of the dense tiling has ONE set (d_slabtilegroup: the set of every 32 rows)
// and its second pass reads that set's W_aer; the live-column tilings (columns with one slab) read the set of their column
// (d_mixgroup).
static int apply_two_pass_rows(sosrt_handle* h, int B) {
    const int L = h->L;
    const std::vector<int>&nz = h->cols.c_nz, &zr0 = h->cols.c_zr0;
    auto zone_end = [&](int b, int z) { return z + 1 < nz[b] ? zr0[b * kMaxZones + z + 1] - 1 : L - 1; };
    const bool sets = h->cols.max_set_used > 0;
    std::vector<int> slab, tileset, colset(B, 0);
    for (int k = 0; k < h->grp.ngroups; ++k) {
        for (int st = 0; st < (sets ? h->phase.nsets : 1); ++st) {
            for (int b = h->grp.gb[k]; b < h->grp.gb[k + 1]; ++b)
                for (int z = 0; z < nz[b]; ++z)
                    if (h->cols.c_zmix[b * kMaxZones + z] && (!sets || h->cols.c_zset[b * kMaxZones + z] == st)) {
                        for (int t = zr0[b * kMaxZones + z]; t <= zone_end(b, z); ++t) slab.push_back(b * L + t);
                        colset[b] = st;
                    }
            if (sets) {
                while (slab.size() % 64) slab.push_back(-1);
                while (tileset.size() < slab.size() / 32) tileset.push_back(st);
            }
        }
        h->grp.slab_off[k + 1] = (int)slab.size();
    }
    if (!slab.empty()) HIPCHK(hipMemcpy(h->cols.d_slabrows, slab.data(), slab.size() * sizeof(int), hipMemcpyHostToDevice));
    if (sets) {
        if (!tileset.empty()) HIPCHK(hipMemcpy(h->cols.d_slabtilegroup, tileset.data(), tileset.size() * sizeof(int), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->cols.d_mixgroup, colset.data(), B * sizeof(int), hipMemcpyHostToDevice));
    }
    h->cols.nslab = (int)slab.size();
    h->cols.mix_groups = 0;
    h->cols.mix_dirty = true;
    h->phase.w32_dirty = true;
    return 0;
}

extern "C" {

int sosrt_set_aerosol_sets(sosrt_t* h, int B, int nzmax, const int* zone_set) {
    if (!h || !zone_set) return fail(SOSRT_E_INVALID, "null argument");
    if (nzmax < 1 || nzmax > kMaxZones) return fail(SOSRT_E_INVALID, "nzmax must be in 1..%d (got %d)", kMaxZones, nzmax);
    if (B < 1) return fail(SOSRT_E_INVALID, "B=%d must be >= 1", B);
    if (!h->have_phase) return fail(SOSRT_E_STATE, "sosrt_set_phase has not been called");
    if (int e = need_gpu(h)) return e;
    if (!h->have_cols) return fail(SOSRT_E_STATE, "sosrt_set_columns has not been called");
    if (B != h->B) return fail(SOSRT_E_INVALID, "B=%d does not match sosrt_set_columns (B=%d)", B, h->B);
    if (h->geom != SOSRT_GEOM_THREE_ZONE) return fail(SOSRT_E_INVALID, "aerosol sets need the three-zone geometry (a single slab has no aerosol)");
    if (h->cols.rw_on) return fail(SOSRT_E_STATE, "sosrt_set_aerosol_sets groups the slab rows again: clear the per-level weights first (sosrt_set_row_weights_dev)");
    // nzmax = 1: one set per column, for each of its aerosol zones; else one per zone of the caller's table
    std::vector<int> zset((size_t)B * kMaxZones, 0);
    int top = 0;
    for (int b = 0; b < B; ++b) {
        if (nzmax > 1 && h->cols.c_nz[b] > nzmax) return fail(SOSRT_E_INVALID, "column %d has %d zones, nzmax is %d", b, h->cols.c_nz[b], nzmax);
        for (int z = 0; z < h->cols.c_nz[b]; ++z) {
            if (!h->cols.c_zmix[b * kMaxZones + z]) continue;           // entries of clear zones are ignored
            const int st = nzmax == 1 ? zone_set[b] : zone_set[b * nzmax + z];
            if (st < 0 || st >= h->phase.nsets)
                return fail(SOSRT_E_INVALID, "column %d zone %d: aerosol set %d outside 0..%d (sosrt_set_phase_sets)", b, z, st, h->phase.nsets - 1);
            zset[b * kMaxZones + z] = st;
            top = st > top ? st : top;
        }
    }
    MixGroups mg;
    const int cap = mix_group_cap(h, top > 0 || h->cols.max_atm_used > 0);
    // (beyond the cache the slab rows take two passes, W_atm and then the W_aer of their set: apply_two_pass_rows)
    const bool fits = collect_mix_groups(h, B, zset, h->cols.c_atmset, cap, mg);
    if (!fits && h->cols.max_atm_used > 0)
        return fail(SOSRT_E_INVALID, "more than %d distinct (atmosphere set, aerosol set, ca, cr) groups: the two-pass form that a batch beyond the "
                                     "cache takes reads one W_atm, and the current columns use atmosphere sets", cap);
    const bool regroup = top > 0 || h->cols.max_set_used > 0;      // (all on set 0 before and after: the groups sosrt_set_columns built stand)
    h->cols.c_zset = zset;
    h->cols.max_set_used = top;
    h->cols.p0_zones = nzmax > 1 ? nzmax : 0;
    if (regroup && (!fits || !mg.ca.empty())) {
        HIPCHK(hipSetDevice(h->device));
        HIPCHK(hipStreamSynchronize(h->stream));
        if (int e = fits ? apply_mix_groups(h, B, mg) : apply_two_pass_rows(h, B)) return e;
    }
    return 0;
}

int sosrt_set_atmosphere_sets(sosrt_t* h, int B, const int* col_set) {
    if (!h || !col_set) return fail(SOSRT_E_INVALID, "null argument");
    if (B < 1) return fail(SOSRT_E_INVALID, "B=%d must be >= 1", B);
    if (int e = need_gpu(h)) return e;
    if (!h->have_phase) return fail(SOSRT_E_STATE, "sosrt_set_phase has not been called");
    if (!h->have_cols) return fail(SOSRT_E_STATE, "sosrt_set_columns has not been called");
    if (B != h->B) return fail(SOSRT_E_INVALID, "B=%d does not match sosrt_set_columns (B=%d)", B, h->B);
    std::vector<int> aset(col_set, col_set + B);
    int top = 0;
    for (int b = 0; b < B; ++b) {
        if (aset[b] < 0 || aset[b] >= h->phase.natm)
            return fail(SOSRT_E_INVALID, "column %d: atmosphere set %d outside 0..%d (sosrt_set_atm_phase_sets)", b, aset[b], h->phase.natm - 1);
        top = aset[b] > top ? aset[b] : top;
    }
    if (top == 0 && h->cols.max_atm_used == 0) return 0;      // all on set 0 before and after: nothing to do
    if (h->cols.rw_on) return fail(SOSRT_E_STATE, "sosrt_set_atmosphere_sets groups the slab rows again: clear the per-level weights first (sosrt_set_row_weights_dev)");
    if (top > 0) {
        // (what sosrt_set_atm_phase_sets accepted S_atm > 1 under; sosrt_set_contraction / sosrt_set_first_order keep it so)
        if (!use_lowrank(h) || !use_sym(h))
            return fail(SOSRT_E_INVALID, "atmosphere sets need the low-rank plain rows and the flip-symmetric form of SOSRT_CONTRACT_F64");
        if (h->first_order_mode == SOSRT_FIRST_ORDER_README)
            return fail(SOSRT_E_INVALID, "SOSRT_FIRST_ORDER_README reads one atmosphere matrix: it cannot be combined with atmosphere sets");
    }
    const bool slabs = h->geom == SOSRT_GEOM_THREE_ZONE && h->cols.nslab > 0;
    MixGroups mg;
    bool fits = true;
    if (slabs) {
        const int cap = mix_group_cap(h, top > 0 || h->cols.max_set_used > 0);
        fits = collect_mix_groups(h, B, h->cols.c_zset, aset, cap, mg);
        if (!fits && top > 0)
            return fail(SOSRT_E_INVALID, "more than %d distinct (atmosphere set, aerosol set, ca, cr) groups: the two-pass form that a batch beyond the "
                                         "cache takes reads one W_atm, so it is not available with atmosphere sets", cap);
    }
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(h->cols.d_colatm, aset.data(), B * sizeof(int), hipMemcpyHostToDevice));
    h->cols.c_atmset = aset;
    h->cols.max_atm_used = top;
    h->resident = false;
    if (slabs)
        if (int e = fits ? apply_mix_groups(h, B, mg) : apply_two_pass_rows(h, B)) return e;
    return 0;
}

// Per-level weights on the row coefficients.  While set the slab rows run the two-pass form, which multiplies
// by the coefficients row by row (a combined matrix has them baked in); clearing restores the grouping the columns had.
int sosrt_set_row_weights_dev(sosrt_t* h, int B, const double* d_w_atm, const double* d_w_aer) {
    if (int e = need_gpu(h)) return e;
    if (!h->have_cols) return fail(SOSRT_E_STATE, "sosrt_set_row_weights_dev: sosrt_set_columns has not been called");
    if (h->geom != SOSRT_GEOM_THREE_ZONE)
        return fail(SOSRT_E_INVALID, "sosrt_set_row_weights_dev: per-level weights are for three-zone and zone-table columns; the single slab "
                                     "(SOSRT_GEOM_SINGLE_SLAB) has no layer-by-layer first order to go with them");
    if (B < 1 || B > h->B) return fail(SOSRT_E_INVALID, "sosrt_set_row_weights_dev: B=%d, the handle's current columns are %d (sosrt_set_columns)", B, h->B);
    const bool on = d_w_atm || d_w_aer;
    if (on && h->cols.max_atm_used > 0)
        return fail(SOSRT_E_INVALID, "sosrt_set_row_weights_dev: the two-pass form that weighted slab rows take reads one W_atm, and the current "
                                     "columns use atmosphere sets (sosrt_set_atmosphere_sets)");
    HIPCHK(hipSetDevice(h->device));
    prof_break(h);
    if (on) {
        // columns B .. of the batch, if any, keep weight one
        const size_t n = (size_t)h->B * h->L;
        if (int e = h->cols.d_rwa.reserve((size_t)h->max_batch * h->L)) return e;
        if (int e = h->cols.d_rwr.reserve((size_t)h->max_batch * h->L)) return e;
        launch_row_weights_copy(h->stream, n, (size_t)B * h->L, d_w_atm, d_w_aer, h->cols.d_rwa.p, h->cols.d_rwr.p);
        HIPCHK(hipGetLastError());
        if (!h->cols.rw_on && h->cols.mix_groups > 0) {
            HIPCHK(hipStreamSynchronize(h->stream));           // (the row lists are rewritten by blocking copies)
            if (int e = apply_two_pass_rows(h, h->B)) return e;
            h->cols.rw_regrouped = true;
        }
        h->cols.rw_on = true;
        return 0;
    }
    if (!h->cols.rw_on) return 0;
    h->cols.rw_on = false;
    if (h->cols.rw_regrouped) {
        h->cols.rw_regrouped = false;
        MixGroups mg;
        const int cap = mix_group_cap(h, h->cols.max_set_used > 0 || h->cols.max_atm_used > 0);
        if (collect_mix_groups(h, h->B, h->cols.c_zset, h->cols.c_atmset, cap, mg) && !mg.ca.empty()) {
            HIPCHK(hipStreamSynchronize(h->stream));
            if (int e = apply_mix_groups(h, h->B, mg)) return e;
        }
    }
    return 0;
}

}  // extern "C"
