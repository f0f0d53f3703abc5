// plan_dev.h — the sorts, scans and first-occurrence numberings of the one-pair tile plan (spcg_plan.cpp
// stages 1-3, 5, 6 and 8) on the device (plan_dev.hip).  Every stage has a unique output — a stable sort from
// ascending ids, component roots that are the smallest id, a first-encounter numbering — so the arrays are the
// host's bit for bit.  With deftri_set_tile_builder the tile layout (spcg_tile.cpp build_tiles, stage 4a)
// is built there too, and with deftri_set_layout_builder the phase-1 blocks and the phase-2 wave layout
// (stages 7 and 8b), whose two slot arrays can stay on the device.  deftri_set_multi_pair_builder opens
// stages 1-3, 5, 6, 8 and 8b to a plan of several pairs, and deftri_set_multi_tile_builder builds its tile
// layout (spcg_tile.cpp build_tiles_multi, stage 4a) there as well.  Both tile layouts are cut by one
// routine, cut_tiles(), over nodes that are groups (one pair) or (pair, group) units (several pairs); which of these
// builders a build uses is one PlanBuilders value, handed to rows() and kept for the calls after it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "../../include/deftri.h"

namespace deftri {

struct SpPlanHost;

constexpr int kPlanScanTile = 2048;      // elements per workgroup of the multi-block scan (256 threads x 8)
constexpr int kPlanRadixTile = 256;      // keys per workgroup of the radix sort (one per thread)
constexpr int kPlanRadixBits = 7;        // digit width: 6 passes over the 42-bit curve key
constexpr int kPlanRunMax = 256;         // longest run (a row's incidences, a group's points) the per-run sort orders
constexpr int kPlanHookRetries = 1024;   // compare-and-swap retries of one union before the build is marked

// the device builders of one build beyond stages 1-3, 5, 6 and 8: what the context's switches ask for
// (build_sp_plan_with), narrowed to what the problem allows (spcg_plan.cpp build_impl), and what rows() lays out.
// tiles: deftri_set_tile_builder; layout: deftri_set_layout_builder, keep_slots: pmap and pidx stay on the device;
// multi: deftri_set_multi_pair_builder and a problem of several pairs; multi_tiles: deftri_set_multi_tile_builder
struct PlanBuilders {
    bool tiles = false, layout = false, keep_slots = false, multi = false, multi_tiles = false;
};

// deftri_plan_build_info
struct PlanBuildInfo {
    int32_t builder_used = 0, stages = 0, reason = 0;
    double ms = 0;
};

// the device arena and the pinned staging of the plan builder, kept across builds (grow-only) on the context
class PlanDevice {
 public:
    PlanDevice(int device, hipStream_t st) : dev_(device), st_(st) {}
    ~PlanDevice();
    PlanDevice(const PlanDevice &) = delete;
    PlanDevice &operator=(const PlanDevice &) = delete;

    // Both return 0, 1 when a bounded loop reached its bound (the caller builds on the host), or -1 with err
    // after a HIP error.
    // stages 1-3 (groups, Morton order, rows) of a validated one-pair problem: one upload of the inputs, the
    // kernels, one download.  before_alloc: called (and cleared) before the arena grows.  on: the builders whose
    // scratch and inputs join the arena (kept for the calls below)
    int rows(const deftri_problem_desc &d, std::function<void()> *before_alloc, int32_t &ng,
             std::vector<int32_t> &point_of_row, std::vector<int32_t> &row_of_point, std::vector<int32_t> &gp,
             std::string &err, PlanBuilders on);
    // deftri_set_multi_pair_builder: rows() with on.multi takes a problem of several pairs and numbers the
    // rows keyframe-major as spcg_plan.cpp stage 3 does for a multi-pair tile plan — by (camera of the point's first
    // reprojection edge, curve key of the point's own position in that camera's box, point) — unless a point's
    // reprojection edges name two cameras, where the group order stays; the choice is made on the device from a
    // flag word.  gp comes back unless on.multi_tiles keeps it for tiles_multi(); on.layout then lays out stage 8b's
    // scratch only, and layout() runs stage 8b alone (ran bits 1 and 2).  Needs n_cams < 2^21
    // stages 4-6 (rotation numbering, rep / depth edges by row, incidences) for H.arap_ids on the rows of the
    // last rows() call: one upload of arap_ids, the kernels, one download into H
    int edges(const deftri_problem_desc &d, SpPlanHost &H, std::string &err);
    // deftri_set_tile_builder: rows() with on.tiles lays out the tile stages' scratch and leaves gp on
    // the device (gp comes back empty).  tiles() is build_tiles (spcg_tile.cpp) of one rank on the rows of the last
    // rows() call: groups and edges by group, the partition, entries and slots, cross slots, then one download of
    // the tile arrays and scalars into H and of the tile-entry order of the ARAP edges into `order`; edges() then
    // takes arap_ids from the device.  units_max / lds_budget: the host's values (sp_tile_units, sp_tile_lds_budget).
    // Returns 0, 1 (bound), -1 (err), or 2: build_tiles would refuse this graph — nothing of H is written and gp
    // is downloaded for the host's build_tiles.  Both tiles() and tiles_multi() are front ends: each points a
    // TileScratch at its own scratch, writes the edges by node and hands the rest to cut_tiles()
    int tiles(const deftri_problem_desc &d, int32_t ng, int units_max, int lds_budget, std::function<void()> *before_alloc,
              SpPlanHost &H, std::vector<int32_t> &order, std::vector<int32_t> &gp, std::string &err);
    // deftri_set_multi_tile_builder: rows() with on.multi and on.multi_tiles uploads arap_pair and dep_scale too
    // and leaves gp on the device.  tiles_multi() is build_tiles_multi (spcg_tile.cpp) on the rows of the last rows()
    // call: the (pair, group) units in each pair's own Morton order, the edges by unit, the partition per pair,
    // entries, slots, own rows and shares, cross slots, then one download of the tile arrays and scalars into H and of
    // the edge order into `order`; edges() then takes arap_ids from the device.  Its scratch is an arena of its own,
    // laid out here because it follows the group count.  Returns as tiles() does; 2 also where a count leaves the int
    // range the kernels index with (build_tiles_multi then runs on the host)
    int tiles_multi(const deftri_problem_desc &d, int32_t ng, int units_max, int lds_budget, std::function<void()> *before_alloc,
                    SpPlanHost &H, std::vector<int32_t> &order, std::vector<int32_t> &gp, std::string &err);
    // deftri_set_layout_builder: rows() with on.layout lays out the scratch of stages 7 and 8b
    // and uploads dep_scale with the other inputs.
    // layout() is those two stages on the arrays edges() left on the device: dperm, blk, hv_blk, hv_blk_off (ran
    // bit 0), the window sort and the wave cut with rowmap, woff and wsplit (bit 1), the slot fill of pmap and pidx
    // (bit 2).  The slot arrays stay on the device (H.pmap_dev, H.pidx_dev, H.slots_dev: valid until the next build
    // on this arena) and come to H.pmap / H.pidx only with download_slots.  When 64 x slots does not fit an int only
    // bit 0 is set and H keeps the host's stage 8b to do.  Returns 0, 1 (bound) or -1 (err)
    int layout(const deftri_problem_desc &d, std::function<void()> *before_alloc, SpPlanHost &H, bool download_slots,
               int32_t &ran, std::string &err);

 private:
    struct TileScratch;                                          // cut_tiles(): the device pointers of its scratch
    struct MultiExtras;                                          // cut_tiles(): what only several pairs add to it
    // the event slots of the DEFTRI_PLAN_TIMING lines: one run per entry point (a context builds one plan at a time)
    // (each run is one event more than its report() has lines).  kEvCut's first event is recorded by the front end,
    // before its edge kernels; cut_tiles() records the other four
    enum { kEvRows = 0,                  // rows(): 5 lines
           kEvEdges = kEvRows + 6,       // edges(): 5 lines
           kEvUnits = kEvEdges + 6,      // tiles_multi(), the unit stage: 2 lines
           kEvCut = kEvUnits + 3,        // tiles() / tiles_multi() then cut_tiles(), up to the counts: 4 lines
           kEvFill = kEvCut + 5,         // cut_tiles() after the counts: 3 lines
           kEvLayout = kEvFill + 4,      // layout(), stages 7 and 8b: 3 lines
           kEvSlots = kEvLayout + 4,     // layout(), the slot fill: 2 lines
           kEvCount = kEvSlots + 3 };
    bool reserve(size_t dev_bytes, size_t pin_bytes, std::function<void()> *before_alloc);
    // synchronizes the stream and picks up a launch error; false with err = "plan builder (<what>): <hip string>"
    bool sync(const char *what, std::string &err);
    // the graph is the host's to cut: gp to the host; returns 2, or -1 with err
    int refuse(std::vector<int32_t> &gp, const char *what, std::string &err);
    // the tile layout over n nodes from the edges by node (s.egi, s.egj, s.erow, written after the event kEvCut): edges
    // by node, the partition, the counts and their download, the tile arena, entries and slots, cross slots, the
    // download into H and `order`.  mx: null for one pair.  Returns as tiles() does
    int cut_tiles(const TileScratch &s, const MultiExtras *mx, int32_t n, int units_max, int lds_budget,
                  std::function<void()> *before_alloc, SpPlanHost &H, std::vector<int32_t> &order, std::vector<int32_t> &gp,
                  std::string &err);
    // part / cur: the scratch of the scan's tile sums and of the fill's cursors (null: the arena's own pieces)
    void scan(int *data, int64_t n, int *part = nullptr);
    void sort_by_row(int64_t n, const int *key, int32_t nkeys, int *off, int *out, int *hdr, int *cur = nullptr, int *part = nullptr);
    int radix_sort(uint64_t *const key[2], int *const id[2], int *hist, int *part, const int *np, int ntile, int passes);
    void report(int first, int last, const char *const *names) const;
    int dev_;
    hipStream_t st_;
    char *buf_ = nullptr, *pin_ = nullptr, *tbuf_ = nullptr;     // tbuf_: the tile arrays of cut_tiles (sized after the counts)
    char *sbuf_ = nullptr;                                       // the slot arrays pmap | pidx (sized after the cut)
    char *mbuf_ = nullptr;                                       // the scratch of tiles_multi (sized by the units)
    size_t cap_ = 0, pin_cap_ = 0, tcap_ = 0, scap_ = 0, mcap_ = 0;
    hipEvent_t ev_[kEvCount] = {};
    // the arena's pieces (byte offsets), laid out by rows()
    struct Layout {
        size_t ap, rot, rep_point, dep_point, xy, par, root, flag, gid, grep, mm, lohi, key[2], id[2], hist, gpos, cur,
            part, dl1, hdr, por, rop, gp, dl1_end, aid, rv, first, rflag, kr, kd, ki, ioff, dl2, hdr2, rot_ids, arl, rep_ids,
            rep_off, dep_ids, dep_off, inc, inc_off, dl2_end,
            // the tile stages' scratch (on.tiles)
            egi, egj, erow, ooff, oe, okj, pred, tioff, ie, tend, ja, jb, mark, midx, tstart, tne, tnh, tcut, thdr,
            // stages 7 and 8b (on.layout); dl3 .. dl3_end is their download
            dscale, dflag, bkey, boff, bord, blk0, order, scnt, wnext, wsteps, wsp, wja, wjb, wmark, widx, wsoff, dl3, lhdr,
            dperm, blk, hvb, hvoff, rowmap, woff, wsplit, dl3_end,
            // the keyframe-major rows of several pairs (on.multi)
            pxy, rcam, rfirst, pcam, cbox,
            // arap_pair and dep_scale for tiles_multi (on.multi_tiles; mdscale is dscale where on.layout laid it out)
            mpair, mdscale, total;
    } L_{};
    PlanBuilders on_;                                          // what the last rows() laid out (keep_slots: unused here)
    bool order_on_dev_ = false;                                // cut_tiles() left arap_ids at order_dev_
    const int *order_dev_ = nullptr;
    int32_t P_ = 0;
    int64_t E_ = 0, nloc_ = -1;                                // nloc_: the local edges of the last edges(), -1 none
};

}  // namespace deftri
