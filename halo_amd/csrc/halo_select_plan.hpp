// Host-side interface between the two selector translation units: halo_select.hip owns the C entry point
// and the serial kernel, halo_select_binned.hip the value-binned sweep.
#pragma once
#include "halo_select_common.hpp"

namespace halo {

// The candidates are placed and swept in two tranches.  kneed = n_regions x window is the proven bound on what the greedy rule can
// visit, reached only when every pick's whole window ranks above the next pick; on real maps the sweep consumes a few candidates per
// pick.  The first tranche therefore holds the top kfirst = min(kneed, n_regions x TRANCHE_F) values, and the rest of the top kneed is
// placed and swept (round B) only for an image whose first tranche ran out short of n_regions picks.  TRANCHE_F: twice the largest
// consumed / n_regions measured on the bench's data sets, rounded up to a power of two (NOTES round 30); never a correctness matter.
constexpr unsigned TRANCHE_F = 16;

inline unsigned long long tranche_first(unsigned long long kneed, unsigned long long n_regions)
{
    return kneed < n_regions * TRANCHE_F ? kneed : n_regions * TRANCHE_F;
}

struct BinGeom {
    int H, W, n_regions, arad, mrad;
    unsigned kneed, kfirst, captot, target, nfmax;
    int cs, gcy, gcx, gstride;   // pick grid: cell size mrad+1, padded row stride in bytes
    unsigned cmul;               // ceil(2^32 / cs): x / cs == mulhi(x, cmul) for x < 65536
    unsigned grid_bytes;
};

// Plan of one call: geometry, capacities and the workspace carve-up (offsets in bytes).
struct BinPlan {
    bool ok;                     // false: the sweep does not serve this geometry (serial kernel only)
    BinGeom g;
    size_t zero_bytes, total_bytes, lds_bytes;
    size_t off_hdr, off_hist1, off_fcur, off_okmin, off_okmax, off_cbase, off_cm, off_ckey, off_cpos, off_plist;
};

BinPlan binned_plan(int64_t B, int64_t H, int64_t W, int64_t n_regions, int64_t arad, int64_t mrad);

// Enqueue the binned selector.  Images it could not finish are marked SEL_BAIL in their SelHdr
// (`*hdr_out`, B entries) for the serial kernel to continue.
int binned_select(void *score, int dtype, int64_t B, const BinPlan &p, uint8_t *active, uint8_t *selected, int64_t *active_mask,
                  const int64_t *gt, double *picks, int32_t *n_picked, void *workspace, size_t workspace_bytes, hipStream_t st,
                  SelHdr **hdr_out, const void *score_range = nullptr, int32_t *handover = nullptr);

// Per-image counters of the last binned_select on this workspace -> stats (B, 3) int32: {candidates placed, candidates in the
// chunks the sweep processed, sweep rounds run}.  Enqueued on the stream; zeros where the sweep did not run.
int binned_stats(int64_t B, const BinPlan &p, const void *workspace, size_t workspace_bytes, int32_t *stats, hipStream_t st);

// Exact value range of B score maps (hw pixels each) as range records (one SelHdr-sized record per image).
int score_range_exact(const void *score, int dtype, int64_t B, int64_t hw, void *range_out, hipStream_t st);

}  // namespace halo
