// vct_internal.h — context object and kernel launchers behind include/vct.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>
#include <string>
#include <vector>
#include "../../include/vct.h"
#include "vct_device.h"
#include "vct_variants.h"

namespace vct {

// Device-resident state of one context.  Everything lives in HBM for the life
// of the context; nothing is re-allocated per frame.
struct Grid {
    uint32_t n = 0, L = 0;
    int aniso = 1;
    float g0[3] = {0, 0, 0};
    float extent = 1.0f;
    float inv_h = 1.0f;
    // radiance pyramid: ONE allocation, level 0 (isotropic) then levels 1..L,
    // each level = faces x n_l^3 float4 texels, linear-Z inside a face volume.
    float4* pyr = nullptr;
    uint64_t lvl_off[kMaxLevels + 1] = {};   // float4 offset of each level
    uint64_t pyr_texels = 0;
    // K1 state
    long long* accum = nullptr;      // [n^3][8] int64: albedo rgb, normal xyz, count, pad
    bool accum_packed = false;       // the last K1 packed its sums (r+2^32 g, b+2^32 nx, ny+2^32 nz, count)
    uint32_t k1_maxabs = 0;          // largest |16.16 value| a hit of the last K1 pass added (clamped at 2^31;
                                     // 0 after a load): the dynamic layer's packed-sum rule needs the static pass's
    float4* albedo_occ = nullptr;    // [n^3] (albedo rgb, occupancy)
    float4* normal = nullptr;        // [n^3] (unit normal, 0)
    unsigned long long* occ_bits = nullptr;  // [n^3 / 64] occupancy bitmask
    uint32_t* occ_list = nullptr;            // [n^3] the occupied voxels of the last K1 (k2_list order)
    uint32_t* occ_count = nullptr;           // [1] entries of occ_list
    // K4 empty-space maps (vct_mips.hip, rebuilt by every build_mips): b0 = one bit per
    // level-0 texel, set iff the texel is not +0 (bit order = the texel's index in the brick
    // layout, so byte v = the eight children of level-1 texel v); occ = per level m >= 2 one
    // byte per texel, nonzero iff some level-0 texel under it is; zmap = per level m = 0..zm_levels
    // one bit per position p in [-1, n_m - 1]^3 (stored at p + 1), set iff any level-m texel of
    // p + {0,1}^3 may be nonzero (texels outside the level are zero).  A level-l trilinear
    // footprint at corner c is exactly the texels c + {0,1}^3, so a clear bit of map l at c
    // proves the footprint's texels (every face) are +0 (zm_sh = 0, the exact test).  It also
    // lies under the level-(l+1) texels c >> 1 + {0,1}^3, so a clear bit of map l+1 at c >> 1
    // proves the same for the 4^3 aligned region around it (zm_sh = 1, the coarse test).
    // Map 0 (from b0; 2.3 MB at 256^3, 18 MB at 512^3) is only kept for n <= kZMap0MaxN:
    // above that, level 0 keeps the coarse test whatever zm_sh says.
    static constexpr int kZLevels = 5;
    static constexpr uint32_t kZMap0MaxN = 512;
    uint32_t* b0 = nullptr;                  // [n^3 / 32]
    uint8_t* occ = nullptr;                  // levels 2..zm_levels, byte per texel, back to back
    uint64_t occ_off[kZLevels + 1] = {};     // byte offset of level m in occ (m >= 2)
    uint32_t* zmap = nullptr;                // maps 1..zm_levels back to back, then map 0
    uint32_t zm_off[kZLevels + 1] = {};      // dword offset of map m
    uint32_t zm_dim[kZLevels + 1] = {};      // n_m + 1 positions per axis (zm_dim[0] = 0: no map 0)
    uint32_t zm_rw[kZLevels + 1] = {};       // dwords per row of map m
    uint32_t zm_words = 0;                   // dwords of zmap
    int zm_levels = 0;
    int zm_sh = 0;                           // 0: exact test, 1: coarse (VCT_ZMAP_EXACT=0), set by build_mips
    bool zm_valid = false;                   // the maps describe the current pyramid
    // Relight builds (vct_mips.hip launch_mips): after K2, level 0 is nonzero exactly at
    // the occupied voxels (every one gets alpha 1, every other voxel is +0), a pattern only
    // K1 changes.  k3_live[b] = 1 iff K3's first-launch block b (k3_live_bz its depth)
    // holds an occupied voxel.  k3_sparse_ok: the last K3 build ran on such a level 0 for
    // the current occupancy, so every level >= 1 texel and b0 bit above a non-live block is
    // +0 / 0 and the K4 maps are current; the next build from a K2 level 0 may then skip
    // the non-live blocks and the maps.  Cleared by K1 and by any dense level-0 write.
    uint8_t* k3_live = nullptr;              // [n^3 / 256] live flag per block
    uint32_t* k3_live_list = nullptr;        // [n^3 / 1024] + count: the live blocks (any order)
    uint32_t k3_live_count = 0;              // host copy, read back with K1's error word
    int k3_live_bz = 0;
    bool k3_sparse_ok = false;
    // K2's coarse occupancy bits (one per brick of (n/64)^3 voxels, 64-bit rows): from K1's
    // occupancy, so built by the first K2 after each K1 and reused by the next ones
    uint32_t* k2_coarse = nullptr;           // [2 * 64 * 64]
    bool k2_coarse_ok = false;
    bool voxelized = false, injected = false, mipped = false;
    bool l0_dense = false;   // level 0 was replaced densely (upload / device copy): K2 must clear it whole
    bool l0_on_peers = false;   // multi-device: the other devices hold this level 0 (vct_build_mips copies it)
    bool bounced = false;       // vct_inject_bounces has added to this level 0 (cleared with every new level 0)
    bool emitted = false;       // vct_inject_emission has added to this level 0 (cleared where bounced is)
    bool skied = false;         // vct_inject_sky has added to this level 0 (cleared where bounced is)
    uint64_t mips_serial = 0;   // bumped by every mip build (launch_mips): with `mipped`, the identity of
                                // the pyramid that vct_build_fog stamps its volume with
};

// Emissive surfaces (vct_emission.hip; vct_spec.h "emissive surfaces").  The emission grid
// E of the current voxelization, sparse: one bit per voxel, the number of emissive voxels
// before each 64-voxel word, and the emissive voxels' index and E in bitmask order, so
//     rank(v) = prefix[v >> 6] + popc(bits[v >> 6] & ((1ull << (v & 63)) - 1))
// finds a voxel's entry in O(1).  The integer sums are accumulated per OCCUPIED voxel
// (rank among K1's occupancy bits: a hit outside them is dropped), so nothing here is sized
// by n^3 but the bit and prefix words (3 n^3 / 16 bytes).  Allocated by the first
// vct_voxelize_emission*, grown when a voxelization occupies more voxels.
struct Emission {
    unsigned long long* bits = nullptr;   // [n^3 / 64] emissive voxels
    uint32_t* prefix = nullptr;           // [n^3 / 64] emissive voxels before word w
    long long* sums = nullptr;            // [cap][3] S rgb per occupied voxel (occupancy rank)
    uint32_t* vox = nullptr;              // [cap] linear-Z voxel of entry i (entries < *count)
    float4* E = nullptr;                  // [cap] (E rgb, 1) of entry i
    uint32_t* count = nullptr;            // [1] emissive voxels (device)
    size_t cap = 0;                       // entries sums / vox / E hold
    bool built = false;                   // E belongs to the voxelization `epoch` (else: empty)
    bool maybe = false;                   // built, and some triangle had candidates (the count may be > 0)
    uint32_t epoch = 0;                   // vct_ctx::grid_epoch of the build
    int64_t n_host = -1;                  // the count once read back (vct_emission_voxels), -1 unknown
};

// The dynamic layer (vct_dynamic.hip; vct_spec.h "dynamic layer").  K1's state is integer
// sums, so a triangle's contribution can be subtracted exactly: the context keeps the
// current layer's per-triangle setup records (120 bytes each) and the bit mask of the voxels
// it hit, and an update retracts them and adds the new layer's.  Two record sets, swapped by
// every update.  The record belongs to the grid of epoch `epoch`: any other voxelization or
// load bumps vct_ctx::grid_epoch and thereby drops it (the grid it leaves is the static one).
struct DynLayer {
    void* rec = nullptr;                  // geom | fix | offsets of `cap` triangles, then the head (device)
    size_t cap = 0;                       // triangles `rec` holds
    uint32_t n_tri = 0;
    unsigned long long total = 0;         // candidates (host copy of the head's)
    unsigned long long* bits = nullptr;   // [n^3 / 64] voxels the layer hit
};
struct Dynamic {
    DynLayer layer[2];
    int cur = 0;                          // the layer in place; 1 - cur is built by the next update
    bool live = false;                    // a record exists ...
    uint32_t epoch = 0;                   // ... for the grid of this vct_ctx::grid_epoch
    uint32_t n_static = 0;                // triangles of Mesh::tri that are the static scene's
    uint32_t n_voxels = 0;                // voxels the layer in place hits (vct_dynamic_voxels)
    void* h_head = nullptr;               // pinned host copy of an update's read-back (counts, error word)
};

// The object set (vct_objects.hip; vct_spec.h "dynamic objects").  Rigid meshes registered once
// in object space and placed by a matrix per object; an update retracts and re-adds the records
// of the objects it names and of no other.  Per triangle of the set the context keeps K1's setup
// record for the pose in place (TriGeom, the six 16.16 values, the candidate count: 120 bytes),
// so a retraction needs neither the old pose nor the mesh.  Object k's triangles are
// [first[k], first[k + 1]) of the set and sit behind the static ones in Mesh::tri.  Like the
// layer's, the records belong to the grid of epoch `epoch`: an update carries them to the epoch
// it makes, any other voxelization or load drops them.
struct Objects {
    bool live = false;                    // a set is defined ...
    uint32_t epoch = 0;                   // ... for the grid of this vct_ctx::grid_epoch
    uint32_t n_static = 0;                // triangles of Mesh::tri that are the static scene's
    uint32_t n_objects = 0, n_tri = 0, n_visible = 0;
    uint32_t maxabs = 0;                  // largest |16.16 value| the set ever added (the packed-sum rule)
    std::vector<uint32_t> first;          // [n_objects + 1] triangle range of each object
    float* pos = nullptr;                 // packed object-space positions, 3 floats a vertex (device)
    uint32_t* idx = nullptr;              // [3 n_tri] indices into pos
    uint32_t* mat = nullptr;              // [n_tri] material ids
    float4* kd = nullptr;                 // [n_mat] the set's table (nullptr: albedo 1)
    uint32_t n_mat = 0;
    void* rec = nullptr;                  // geom | fix | counts of n_tri triangles, then the head (device)
    uint32_t* vis = nullptr;              // [n_objects] 1 = visible
    void* poses = nullptr;                // [n_objects] vct_object_pose: the last pose given to each, all zero before
    uint32_t* d_first = nullptr;          // [n_objects + 1] `first` on the device (vct_motion.hip)
    unsigned long long* mask = nullptr;   // [n^3 / 64] voxels an update hit; all zero between updates
    void* tab = nullptr;                  // an update's table: prefix, first triangle and id per named object,
    void* h_tab = nullptr;                // then the poses (device; pinned host staging of the same layout)
    void* h_head = nullptr;               // pinned host copy of an update's read-back
    uint32_t last_moved = 0, last_touched = 0;
    unsigned long long last_cand = 0;
};

struct Mesh {
    float4* tri = nullptr;        // [n_tri][4] : v0, e1 = v1-v0, e2 = v2-v0, (kd rgb, diffuse map as int bits; -1 none)
    float4* uv = nullptr;         // [n_tri][2] : (u0 v0 u1 v1), (u2 v2 0 0)  (textured voxelizations)
    uint32_t n_tri = 0;
    size_t cap = 0, uv_cap = 0;
    bool textured = false;        // the last voxelization had mapped materials (uv is valid)
};

// diffuse maps of vct_set_textures (vct_spec.h "diffuse maps")
struct Textures {
    uint32_t* texels = nullptr;   // every texture's RGBA8 texels, back to back
    TexDesc* desc = nullptr;      // [n] offset / size
    uint32_t n = 0;
    size_t texel_cap = 0, desc_cap = 0;
};

struct Scratch {
    void* p = nullptr;
    size_t bytes = 0;
};

// Light bounces (vct_bounce.hip; vct_spec.h "light bounces").  The sources of a
// voxelization -- occupied voxels with a nonzero normal -- are kept as a materialised
// G-buffer that K4 traces like a frame of 64 * tiles_x by 64 * tiles_y pixels: source s
// sits at the pixel that lane s % 64 of K4's unit s / 64 traces (bounce_pixel), so a wave
// holds 64 consecutive sources, and the sources are listed region by region (16^3 voxels,
// Morton order inside), so those 64 are neighbours.  Pixels past the last source are
// background records (P.w = 0).  84 bytes per source: position, normal, K4's two outputs,
// the level 0 the bounces add to, and the voxel index.  Built on the first use after a
// voxelization or load (one count is read back), reused by every relight.
struct Bounce {
    bool built = false;
    uint32_t epoch = 0;              // vct_ctx::grid_epoch the list belongs to
    uint32_t n_src = 0;
    uint32_t tiles_x = 0, tiles_y = 0;
    uint32_t* vox = nullptr;         // [n_src] linear-Z voxel of source s
    float4* l0 = nullptr;            // [n_src] level 0 before the first bounce
    float4* gbuf = nullptr;          // [4][px]: position, normal, diffuse out, specular out
    uint32_t* region = nullptr;      // [regions + 1] sources per region, then their prefix sums
    size_t src_cap = 0, l0_cap = 0, px_cap = 0, region_cap = 0;
    int form = 0;                    // the compiled K4 form the gather launches (0 union, 1 occupancy;
                                     // atrium 256^3: 0.754 against 0.791 ms, tools/bounce_bench.py)
    int order = 1;                   // 1 region runs, 0 occ_list order (vct_debug_bounce, A/B: 0.754
                                     // against 1.534 ms per gather)
    bool profile = false;            // vct_debug_bounce: time the stages with events
    hipEvent_t ev[4] = {};
    float ms[4] = {0, 0, 0, 0};      // list build, gather, accumulate, K3 of the last bounce
};

// Volumetric fog (vct_fog.hip; vct_spec.h "volumetric fog").  The scatter volume of the last
// vct_build_fog: m^3 float4 cells in the pyramid's brick layout (vct_device.h texel_index), so
// a 2x2x2 trilinear footprint lies in one to eight 128-byte bricks.  It belongs to the pyramid
// of mip build `serial` of voxelization `epoch`: any level-0 change clears Grid::mipped and any
// mip build bumps Grid::mips_serial, either of which makes it stale.  `gbuf` holds the
// synthetic G-buffer of the ambient term: position, normal and K4's two outputs for 2 m^3
// records (normal +y, then -y).
struct Fog {
    float4* vol = nullptr;
    size_t cap = 0;                  // cells `vol` holds
    uint32_t m = 0, level = 0;
    bool built = false;
    uint32_t epoch = 0;
    uint64_t serial = 0;
    float4* gbuf = nullptr;
    size_t gbuf_cap = 0;             // records per plane
    int path = 0;                    // address path of the last light-cone march: 32 or 64
    unsigned long long* dbg_light_steps = nullptr;     // vct_debug_fog (tools): device counters the builds
    unsigned long long* dbg_ambient_steps = nullptr;   // add their light-cone / ambient K4 steps to
};

// The environment-map sky (vct_env.hip; vct_spec.h "environment sky").  The map of the last
// vct_set_env with its mip chain, one allocation: level j is (size >> j)^2 float4 texels, row
// major, row 0 = p.y = -1, starting at texel 4 (size^2 - (size >> j)^2) / 3 (the levels back to
// back).  Replaced as a whole, after the ctx stream has drained.
struct Env {
    float4* map = nullptr;
    uint32_t size = 0, lg = 0;       // size 0: no map
    int path = 0;                    // address path of the last env march: 32 or 64 (vct_debug_env_path)
    bool profile = false;            // vct_debug_env_mips: time the mip build of vct_set_env with events
    float mip_ms = 0.0f;             // the mip kernels of the last timed vct_set_env
};

// The shading set (vct_shading.hip; vct_spec.h "shading attributes").  Per static triangle one
// record of nine float4 -- per vertex k (normal_k, u_k), (tangent_k, v_k), (bitangent_k, word_k)
// with word_0 = the material index, word_1 = the kShade* presence bits, word_2 = 0 -- so every
// fetch of the pass is one 16-byte load, and the material table as the host gave it (32 bytes a
// material).  It belongs to the static triangles of the voxelization `epoch`; a dynamic update
// carries a live set over to its new epoch (vct_dynamic.hip), every other voxelization or load
// drops it.
struct Shading {
    float4* rec = nullptr;           // [n_tri][9]
    float4* mats = nullptr;          // [n_mat][2]
    size_t rec_cap = 0, mat_cap = 0; // bytes
    uint32_t n_tri = 0, n_mat = 0;
    bool live = false;
    uint32_t epoch = 0;
};

// The cutout table of the mesh (vct_cutout.hip; vct_spec.h "cutouts").  Per static triangle one
// word pair for the G-buffer pass: x = the mask word 4 * mask map + channel (0xFFFFFFFF: opaque),
// y = the cutoff's bits; the TexCoords of every masked triangle are in Mesh::uv.  It belongs to
// the static triangles of the voxelization `epoch`: a dynamic update carries a live table over to
// its new epoch (vct_dynamic.hip; the layer's triangles lie past n_tri and are opaque), every
// other voxelization or load drops it.
struct Cutout {
    uint2* tri = nullptr;            // [n_tri]
    vct_cutout* table = nullptr;     // [n_mat] the host's table, for K1's triangle setup
    size_t tri_cap = 0, table_cap = 0;   // bytes
    uint32_t n_tri = 0, n_masked = 0;
    bool live = false;
    uint32_t epoch = 0;
};

// K4's per-launch scratch, one set per stream: K4 launches on different streams may run
// concurrently (a host that overlaps consecutive frames), so the cone-split hand-over
// and the ray-reorder buffers belong to the stream, not to the context.
// (vct_mixed.hip adds three: the plane a cone selection does not ask for, the upsample's hole
// mask and row counts, and the frame call's low and hole frames; vct_temporal.hip one: the
// per-wave stats words; vct_motion.hip one: the per-object flags and its per-wave stats words)
enum { kScFlags = 0, kScHand = 1, kScKeys = 2, kScSort = 3, kScOrder = 4, kScUnsel = 5, kScMixUp = 6, kScMixed = 7,
       kScTemporal = 8, kScMotion = 9, kScN = 10 };
struct StreamScratch {
    hipStream_t s = nullptr;
    bool used = false;
    Scratch sc[kScN];
};
constexpr int kStreamSets = 4;

// K4 candidate choice (vct_trace.hip k4_form).  The default cone trace has two
// bit-identical compiled forms: the four-face-union form (4 waves/SIMD; pays on curved
// surfaces, where a wave's lanes straddle an axis) and the occupancy form (5 waves/SIMD,
// three-face bricks; pays on flat ones); a one-rank full frame may also be traced in
// screen order or with ray reordering (pays on incoherent G-buffers).  Candidate
// c = form | reordered << 1, over the dimensions the variant leaves open.
//
// One entry per workload (frame size, tiling, cone set, grid size, forced bits), kept in
// a small LRU table so that a host alternating workloads (two G-buffers, counting and
// plain launches, two frame sizes) keeps every choice.  A new entry times each candidate
// on its first counter-free launches (HIP events on the ctx stream; while timing, a
// launch first waits for the previous timed launch of that entry, so the choice is made
// within ~7 launches even when the host queues frames far ahead), then keeps the
// fastest.  After that the launch path never blocks: every kWatchEvery-th launch of the
// chosen candidate is timed with an event pair polled by hipEventQuery.  The entry times
// its candidates again only when (a) kDriftRuns consecutive samples run more than kDrift
// times the settled time (the G-buffer or the scene changed what is fastest), or (b) a
// new voxelization (scene) has happened and the entry has run `epoch_wait` launches
// since its last timing; epoch_wait starts at kEpochMin and doubles (up to kEpochMax)
// each time such a re-timing keeps the same winner, so a host that re-voxelizes every
// frame re-times rarely once the choice is stable.  A re-timing keeps the first sample
// of each candidate (its code is loaded already) and drops a candidate after one sample
// that is kCompetitive times slower than the best so far: a much slower candidate
// (screen order on an incoherent G-buffer: 6x) costs one frame per re-timing.
// While timed launches alternate streams (a host overlapping frames, vct.h conventions;
// until 64 launches after the last switch) the entries are not watched (a launch's event
// time then includes whatever share of the chip the neighbouring frames took: measured
// false drifts), and a timing launch first waits for the previous launch of any stream.
// VCT_TUNE_LOG=1 prints every decision to stderr.
struct K4Tuner {
    static constexpr int kSlots = 4;          // event pairs in flight per candidate
    static constexpr int kSamples = 2;        // timed samples per candidate after the first (cold) one
    static constexpr int kEntries = 4;        // workloads remembered (LRU)
    static constexpr uint32_t kWatchEvery = 2;
    static constexpr int kDriftRuns = 3;
    static constexpr float kDrift = 1.35f;
    static constexpr uint32_t kEpochMin = 16, kEpochMax = 4096;
    static constexpr float kCompetitive = 1.5f;
    struct Entry {
        uint64_t key = ~0ull;                 // workload the entry belongs to
        uint64_t used = 0;                    // LRU stamp
        int chosen = -1;                      // the candidate kept; -1 still timing
        float settled = 0.0f;                 // chosen candidate's time when it was chosen, ms
        int drift = 0;                        // consecutive slow watch samples
        uint32_t since = 0;                   // launches since the choice
        uint32_t launches = 0;                // timed launches while choosing
        uint32_t retimes = 0;                 // re-timings after the first choice
        uint32_t epoch = 0;                   // vct_ctx::grid_epoch the choice was made on
        uint32_t epoch_wait = kEpochMin;      // launches before a new scene re-times the entry
        int prev = -1;                        // the winner before this timing (-1: none)
        bool by_epoch = false;                // this timing was started by a new scene
        hipEvent_t ev[4][kSlots][2] = {};
        bool busy[4][kSlots] = {};
        int head[4] = {0, 0, 0, 0};
        int seen[4] = {0, 0, 0, 0};           // completed samples (the first one of a first timing is dropped)
        float best[4] = {0.0f, 0.0f, 0.0f, 0.0f};   // fastest completed sample, ms
        hipEvent_t last = nullptr;            // end event of the previous timed launch while timing
        // longest-first dispatch (launch_trace): the chosen candidate's per-unit wave durations,
        // recorded by every timed launch; the next one dispatches each XCD's units longest first
        uint32_t* hist = nullptr;             // [hist_cap] s_memrealtime ticks per unit (device)
        uint32_t hist_cap = 0, hist_units = 0;
        int hist_cand = -1;                   // candidate (form | order) the durations belong to
        bool hist_ok = false;                 // a recording launch has been queued
    };
    Entry e[kEntries];
    int cur = -1;                             // entry of the last launch (vct_trace_form)
    uint64_t clock = 0;
    // concurrent frames: once timed launches have come on two streams, each one records
    // `prev_end`, and a timing launch first waits for it (samples stay isolated)
    static constexpr uint64_t kMultiLaunches = 64;   // a stream switch counts for this many launches
    hipStream_t prev_stream = nullptr;        // the last timed launch's stream (the null stream is one too)
    bool prev_set = false;                    // prev_stream holds a launch's stream
    hipEvent_t prev_end = nullptr;
    // duration buffers outgrown by a larger workload: a launch on another stream may still
    // write them, so they are freed with the context, not in the launch path
    std::vector<uint32_t*> retired;
    uint64_t multi_until = 0;                 // clock value up to which launches count as overlapped
    bool multi = false;                       // clock < multi_until at the last launch
};

}  // namespace vct

struct vct_ctx {
    vct_config cfg{};
    int device = 0;
    int n_cu = 0;                       // the device's compute units (queried on first use)
    hipStream_t stream = nullptr;
    vct::Grid grid;
    vct::Mesh mesh;
    vct::Textures tex;
    vct::Scratch scratch[12];    // reusable scratch (0 trace host staging, 1 voxelize temps,
                                  // 2-3 G-buffer bins, 4 K2 work list, 7 K1 candidate bucket table,
                                  // 8 multi-device tiles / gather, 9 multi-device step counters,
                                  // 10 shadow-cone step tables, 11 occupancy ranks of the emission build,
                                  // which also reuses 1 and 7 as K1 does; the dynamic layer's update
                                  // reuses 1 for its scan temps and 4 for its fix-up list)
    float shadow_tau[VCT_MAX_LIGHTS] = {};   // the apertures whose step tables scratch 10 holds, slot by slot
    uint32_t shadow_taus = 0;                // (vct_shadow.hip; 0: none built yet)
    // The tables are shared by every vct_shadow_cones_device call whatever stream the caller
    // sets: a call on another stream than the previous one first makes its stream wait for that
    // call's end (`shadow_done`, recorded after every march), so a table is never read before
    // the launch that builds it has run, nor rewritten while an earlier march reads it; the
    // event of the last call also covers every earlier one (as xchg_done below).
    hipEvent_t shadow_done = nullptr;
    hipStream_t shadow_stream = nullptr;
    int shadow_path = 0;                     // address path of the last march: 32 or 64 (vct_debug_shadow_path)
    int sky_path = 0;                        // the same of the last sky march (vct_debug_sky_path)
    int sky_view_path = 0;                   // and of the last specular sky march (vct_debug_sky_view_path)
    bool sky_profile = false;                // vct_debug_sky: time the stages of vct_inject_sky with events
    hipEvent_t sky_ev[4] = {};
    float sky_ms[3] = {0, 0, 0};             // march, add and K3 of the last vct_inject_sky
    vct::StreamScratch k4s[vct::kStreamSets];   // K4 hand-over + reorder scratch per stream (k4_scratch)
    vct::K4Tuner k4tune;                // timed-form choice of the default cone trace
    vct::Bounce bounce;                 // source list of vct_inject_bounces
    vct::Emission em;                   // emission grid of vct_voxelize_emission*
    vct::Dynamic dyn;                   // dynamic layer of vct_voxelize_dynamic*
    vct::Objects obj;                   // object set of vct_objects_define
    vct::Fog fog;                       // scatter volume of vct_build_fog
    vct::Env env;                       // map and mips of vct_set_env
    vct::Shading shade;                 // attribute records and materials of vct_set_shading
    vct::Cutout cut;                    // per-triangle masks of vct_voxelize_cutout*
    uint32_t grid_epoch = 0;            // bumped by every voxelization (a new scene for the tuner)
    vct::StepRow* step_tab = nullptr;   // [kMaxStepRows] diffuse-cone step table (device)
    unsigned* spec_keys = nullptr;      // [2 * kSpecSlots]: specular table keys (~0u free), then states
    vct::StepRow* spec_rows = nullptr;  // [kSpecSlots][64] specular step tables (filled by K4)
    const uint32_t* k4_dbg_order = nullptr;   // vct_debug_k4_sched (tools): K4 dispatch order
    uint32_t* k4_dbg_dur = nullptr;           // and per-unit wave durations
    uint64_t k4_lpt_launches = 0;             // launches dispatched longest first (vct_debug_k4_lpt_launches)
    int* k1_err = nullptr;              // device flag of vct_voxelize_device (index out of range)
    // vct_create_multi: this context is device rank 0 and owns one context per
    // further device (ranks 1..n-1); empty for a single-device context
    std::vector<vct_ctx*> peers;
    hipEvent_t ev = nullptr;            // cross-device ordering of the multi-device calls
    // The frame exchanges of trace_multi and vct_comm_trace_frame share scratch slots 8 / 9
    // (and the peers' streams) whatever stream the caller sets: each such call first makes
    // the ctx stream wait for the previous call's end (`xchg_done`, recorded on the stream
    // that call ran on), so frames queued on alternating streams never overlap on the
    // shared buffers; the event of the last call also covers every earlier one
    // (vct_comm_synchronize waits for it).
    hipEvent_t xchg_done = nullptr;
    hipStream_t xchg_stream = nullptr;
    void* comm = nullptr;               // RCCL communicator of vct_comm_init (ncclComm_t), one process per GPU
    int comm_rank = 0, comm_size = 1;
    uint32_t comm_timeout_ms = 300000;  // deadline of every blocking step of vct_comm_* (vct_comm_set_timeout)
    bool own_stream = false;            // stream created by vct_create_multi (destroyed with the ctx)
    std::string err;
};

namespace vct {

// K2 input rule, colour (vct_spec.h): finite, not negative (-0.0f by its sign bit) and
// <= VCT_COLOR_LIMIT, which keeps level 0 finite; nullptr, or what is wrong.  The one check of
// vct_inject_directional, vct_composite_device (vct_capi.cpp) and every light of a list
// (prepare_light, vct_light_terms.h).
inline const char* check_color(const float* color) {
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(color[k])) return "non-finite colour";
        if (!(color[k] >= 0.0f) || std::signbit(color[k])) return "negative colour";
        if (color[k] > VCT_COLOR_LIMIT) return "colour above VCT_COLOR_LIMIT";
    }
    return nullptr;
}

// a failed call: its text for vct_last_error and its status
inline vct_status lfail(vct_ctx* c, vct_status s, const std::string& msg) {
    c->err = msg;
    return s;
}

inline vct_status lhip(vct_ctx* c, hipError_t e, const char* where) {
    return lfail(c, e == hipErrorOutOfMemory ? VCT_ENOMEM : VCT_EDEVICE,
                 std::string(where) + ": " + hipGetErrorName(e) + " (" + hipGetErrorString(e) + ")");
}

// K1 input rule, Kd (vct_spec.h): finite and |Kd| < VCT_KD_LIMIT (a NaN fails the compare)
// (`&`, not `&&`: in a kernel, short-circuit evaluation would make each load wait for the one before it)
__host__ __device__ __forceinline__ bool kd_legal(float r, float g, float b) {
    return ((int)(fabsf(r) < VCT_KD_LIMIT) & (int)(fabsf(g) < VCT_KD_LIMIT) & (int)(fabsf(b) < VCT_KD_LIMIT)) != 0;
}

// The Kd rule on the host, before any launch: the Kd of every material a triangle uses (an
// out-of-range material index is the setup kernel's to report); false: one is illegal
inline bool used_kd_legal(const uint32_t* tri_mat, uint32_t n_tri, const float* kd4, uint32_t n_mat) {
    for (uint32_t t = 0; kd4 && t < n_tri; ++t) {
        const uint32_t m = tri_mat ? tri_mat[t] : 0u;
        if (m >= n_mat) continue;
        const float* k = kd4 + 4 * (size_t)m;
        if (!kd_legal(k[0], k[1], k[2])) return false;
    }
    return true;
}

// The device copies of a host-form voxelization's arrays, freed on every exit: whatever reads
// them must have run by then (the caller waits for the ctx stream)
struct DevTmp {
    void* p = nullptr;
    ~DevTmp() { if (p) (void)hipFree(p); }
};
struct MeshStage {
    DevTmp verts, idx, mat, mats, map;
};

// Allocates them and queues the uploads on the ctx stream.  tri_mat, mats4 (n_mat records of 16
// bytes: Kd or Ke, `mats_name` in the error text) and map (n_mat words) may be NULL
inline vct_status stage_mesh(vct_ctx* c, MeshStage& s, const void* verts, size_t vbytes, const uint32_t* idx,
                             uint32_t n_idx, const uint32_t* tri_mat, const float* mats4, const char* mats_name,
                             const int32_t* map, uint32_t n_mat) {
    const struct { DevTmp& d; const void* src; size_t bytes; const char* name; } a[5] = {
        {s.verts, verts, vbytes, "verts"},
        {s.idx, idx, (size_t)n_idx * 4, "idx"},
        {s.mat, tri_mat, tri_mat ? (size_t)(n_idx / 3) * 4 : 0, "mat"},
        {s.mats, mats4, mats4 ? (size_t)n_mat * 16 : 0, mats_name},
        {s.map, map, map ? (size_t)n_mat * 4 : 0, "map"}};
    hipError_t e;
    for (const auto& x : a)
        if (x.bytes && (e = hipMalloc(&x.d.p, x.bytes)) != hipSuccess)
            return lhip(c, e, (std::string("hipMalloc ") + x.name).c_str());
    for (const auto& x : a)
        if (x.bytes && (e = hipMemcpyAsync(x.d.p, x.src, x.bytes, hipMemcpyHostToDevice, c->stream)) != hipSuccess)
            return lhip(c, e, (std::string("upload ") + x.name).c_str());
    return VCT_OK;
}

// K1
// d_map (device, n_mat entries, may be NULL): diffuse map of each material in c->tex
// (-1 none); uv_offset: byte offset of the TexCoords in a vertex record (read when d_map).
// *d_err (device, zeroed by the caller) collects kK1ErrIndex (an index out of range),
// kK1ErrKd (a triangle's Kd is not finite or |Kd| >= VCT_KD_LIMIT) and
// kK1ErrRedo (packed sums may have overflowed: repeat with packed = false); nothing is
// read back here, so the launch queues without a synchronisation after the candidate count.
constexpr int kK1ErrIndex = 1, kK1ErrRedo = 2, kK1ErrKd = 4;
// the text of a Kd that breaks the K1 input rule, from the host check or the device flag
constexpr const char* kKdMessage = "material_kd4: Kd not finite or |Kd| >= 32768";
// cut (vct_voxelize_cutout*): the pass runs vct_cutout.hip's triangle setup and candidates
// kernels in place of K1's own; everything around them is the same pass
struct CutoutPass {
    const vct_cutout* table;   // device, n_mat entries
    uint2* tri;                // device, n_tri entries: Cutout::tri
};
hipError_t launch_voxelize(vct_ctx* c, const void* d_verts,
                           uint32_t stride, uint32_t n_verts, const uint32_t* d_idx, uint32_t n_tri,
                           const uint32_t* d_mat, const float4* d_kd, uint32_t n_mat, const int32_t* d_map,
                           uint32_t uv_offset, int* d_err, bool packed = true, const CutoutPass* cut = nullptr);
// K1 with cutouts (vct_cutout.hip), called by the pass above.  The records are K1's (TriGeom,
// TriFix, TriUV of vct_voxel_sat.h, which are internal to each translation unit: void* here)
struct K1SetupArgs {
    const char* verts; uint32_t stride, n_verts; const uint32_t* idx; uint32_t n_tri; const uint32_t* mat;
    const float4* kd; uint32_t n_mat; const int32_t* map; uint32_t uv_offset, n_tex; int n;
    float g0x, g0y, g0z, inv_h;
    void *geom, *fix, *tuv;
    unsigned long long* counts;
    float4 *mesh_tri, *mesh_uv;
    int* err;
    uint32_t* maxabs;
};
void launch_cutout_setup(vct_ctx* c, const K1SetupArgs& a, const CutoutPass& cut);
void launch_cutout_candidates(vct_ctx* c, uint32_t blocks, bool packed, const void* geom, const void* fix,
                              const unsigned long long* offs, uint32_t n_tri, const unsigned long long* total,
                              const uint32_t* starts, const void* tuv);
// the table rule of vct_voxelize_cutout* (vct_spec.h "cutouts") on the host: nullptr, or what is wrong
const char* cutout_table_error(const vct_ctx* c, const vct_cutout* table, uint32_t n_mat);
// masked entries of a table (0 for NULL)
uint32_t cutout_masked(const vct_cutout* table, uint32_t n_mat);
// Before a cutout pass: grows Cutout::tri and Cutout::table, queues the table's upload on the ctx
// stream and fills *pass.  The table is dropped (live = false) until cutout_commit
hipError_t cutout_begin(vct_ctx* c, const vct_cutout* table, uint32_t n_mat, uint32_t n_tri, CutoutPass* pass);
// after the pass has succeeded: the table belongs to the current grid_epoch
void cutout_commit(vct_ctx* c, const vct_cutout* table, uint32_t n_mat, uint32_t n_tri);
inline bool cutout_live(const vct_ctx* c) { return c->cut.live && c->cut.epoch == c->grid_epoch; }
void cutout_free(vct_ctx* c);
// grid dumps: K1 records [cnt][7] int64 (albedo rgb, normal xyz sums, count) of the voxels
// d_idx (device) -- read out of the accumulators, or written back into them after the
// previous voxelization's sparse reset (bits, occupied list and resolved voxels rebuilt)
hipError_t launch_k1_gather(vct_ctx* c, const uint32_t* d_idx, uint32_t cnt, long long* d_rec);
hipError_t launch_k1_restore(vct_ctx* c, const uint32_t* d_idx, uint32_t cnt, const long long* d_rec);
// K2
hipError_t launch_inject(vct_ctx* c, float lx, float ly, float lz, float cr, float cg, float cb);
// K3 (and the K4 empty-space maps of Grid::zmap)
hipError_t launch_mips(vct_ctx* c);
// K3's live-block list for the occupancy K1 just built (queued on the ctx stream; the count
// reaches g.k3_live_count at the next stream synchronisation)
hipError_t launch_k3_live(vct_ctx* c);
// one nl^3 face volume between the pyramid's texel layout and linear-Z (vct_device.h)
hipError_t launch_relayout(vct_ctx* c, const float4* src, float4* dst, uint32_t nl, bool to_linear);
// K4
// bounce_form >= 0: the gather of vct_inject_bounces -- the diffuse cone set only, whatever
// cfg.specular says, in that compiled form (0 union, 1 occupancy), screen order, without
// the tuner, the longest-first dispatch or the debug schedule; the tuner's state (and
// vct_trace_form) is left as it was
// cones (vct_mixed.h VCT_CONES_*): the cone sets of the context this launch traces; both of
// a's plane pointers are written whatever it selects (an unselected plane gets K4's value for
// no cones)
hipError_t launch_trace(vct_ctx* c, const vct_trace_args* a, int bounce_form = -1, uint32_t cones = 3u);
// light bounces (vct_bounce.hip): the source list of the current voxelization (built when
// c->bounce is stale; synchronises the ctx stream once to read the count back), the copy of
// level 0 the bounces add to, one gather (K4 over the sources), and level 0 = L0 + A * I
hipError_t bounce_sources(vct_ctx* c);
hipError_t launch_bounce_save(vct_ctx* c);
hipError_t launch_bounce_gather(vct_ctx* c);
hipError_t launch_bounce_accumulate(vct_ctx* c);
// sky light (vct_sky.hip): level 0 += A * Sk at every source, Sk read from the source
// G-buffer's plane `plane` (2 or 3: K4's outputs, free between bounces)
hipError_t launch_bounce_add_plane(vct_ctx* c, int plane);
void bounce_free(vct_ctx* c);
// emissive surfaces (vct_emission.hip): the context's emission grid is the one built for the
// current voxelization, and may hold an emissive voxel; release with the context
inline bool emission_live(const vct_ctx* c) {
    return c->em.built && c->em.epoch == c->grid_epoch && c->em.maybe && c->em.n_host != 0;
}
void emission_free(vct_ctx* c);
// dynamic layer (vct_dynamic.hip): the context holds a layer record for the current grid;
// release with the context
inline bool dynamic_live(const vct_ctx* c) { return c->dyn.live && c->dyn.epoch == c->grid_epoch; }
void dynamic_free(vct_ctx* c);
// object set (vct_objects.hip): the context holds a set for the current grid; release with the
// context.  The set and the layer exclude each other (a layer in place: one with triangles)
inline bool objects_live(const vct_ctx* c) { return c->obj.live && c->obj.epoch == c->grid_epoch; }
inline bool layer_in_place(const vct_ctx* c) { return dynamic_live(c) && c->dyn.layer[c->dyn.cur].n_tri > 0; }
void objects_free(vct_ctx* c);
// vct_motion.hip: poses[ids[j]] = src[j] for the n objects an update named (all device pointers)
void objects_scatter_poses(hipStream_t s, const uint32_t* ids, const void* src, uint32_t n, void* poses);
// the triangles of Mesh::tri that the last vct_voxelize* put there
inline uint32_t static_triangles(const vct_ctx* c) {
    return objects_live(c) ? c->obj.n_static : dynamic_live(c) ? c->dyn.n_static : c->mesh.n_tri;
}
// volumetric fog (vct_fog.hip): the context's scatter volume was built from the current pyramid;
// release with the context
inline bool fog_current(const vct_ctx* c) {
    return c->fog.built && c->grid.voxelized && c->grid.mipped && c->fog.epoch == c->grid_epoch &&
           c->fog.serial == c->grid.mips_serial;
}
void fog_free(vct_ctx* c);
// environment-map sky (vct_env.hip): release with the context
void env_free(vct_ctx* c);
// shading set (vct_shading.hip): the context holds one for the current static triangles;
// release with the context
inline bool shading_live(const vct_ctx* c) { return c->shade.live && c->shade.epoch == c->grid_epoch; }
void shading_free(vct_ctx* c);
// ray reordering (variant 0x8000, vct_reorder.hip): *perm = the frame's pixels sorted by the
// Morton code of their cone origin's voxel, background last (device, w * h entries)
// (perm_spec, nullable: a second order for the specular part, by cell and cone aperture)
hipError_t launch_reorder(vct_ctx* c, const vct_trace_args* a, const uint32_t** perm, const uint32_t** perm_spec);
hipError_t launch_untile(vct_ctx* c, const float4* gathered, uint32_t planes, uint32_t w, uint32_t h,
                         uint32_t world, float4* const* frames, bool packed = false);
// composite + present (row f3)
hipError_t launch_composite(vct_ctx* c, const float4* pos, const float4* nrm, const float4* alb,
                            const float4* diff, const float4* spec, uint32_t w, uint32_t h, const float l[3],
                            const float color[3], float4* lin, uint32_t* rgba8);
// Composite + present for a light list (vct_lights.hip), behind vct_composite_lights_device,
// _shadowed_device and _emissive_device (`what`: the entry point, for the error text): the
// argument checks the three share, in their order; then the caller's own rule; then the light
// list's, and one kernel.  What differs between the entry points:
struct CompositeForm {
    const float* vis = nullptr;        // [n_lights][h][w]
    bool read_vis = false;             // V is read from vis, else walked
    float scale = 0.0f;
    bool emit = false;                 // scale * E of the pixel's voxel is added
    const char* own_error = nullptr;   // the caller's own rule is broken: "<what>: <own_error>" is the error
};
vct_status composite_light_list(vct_ctx* c, const char* what, const float* pos4, const float* nrm4, const float* alb4,
                                const float* diffuse4, const float* spec4, uint32_t w, uint32_t h,
                                const vct_light* lights, uint32_t n_lights, const CompositeForm& form,
                                float* out_linear4, uint32_t* out_rgba8);
// G-buffer
hipError_t launch_gbuffer_binned(vct_ctx* c, const vct_camera* cam, uint32_t w, uint32_t h, float rough,
                                 float4* pos, float4* nrm, float4* alb);
hipError_t launch_raycast(vct_ctx* c, const vct_camera* cam, uint32_t w, uint32_t h, float rough,
                          float4* pos, float4* nrm, float4* alb);

// the "G-buffer input rule" of vct_spec.h on a camera and a frame size (vct_capi.cpp's
// bad_gbuffer_input): nullptr, or what is wrong; cam must not be NULL
const char* gbuffer_input_error(const vct_camera* cam, uint32_t w, uint32_t h);

uint32_t tiles_for_rank(uint32_t w, uint32_t h, uint32_t rank, uint32_t world);
// dst[j] += sum over i < n of src[2 i + j], j = 0, 1 (a NULL dst is skipped): the
// multi-device trace folds the other devices' step / texel counters into the caller's
hipError_t launch_add_counters(vct_ctx* c, const unsigned long long* src, uint32_t n, unsigned long long* dst0,
                               unsigned long long* dst1);

// K4 step table for aperture tau on an n^3 grid (rows until t > n*sqrt(3), then
// one sentinel row with t = +inf); returns the row count incl. the sentinel, or
// -1 if it exceeds kMaxStepRows
int build_step_table(float tau, uint32_t n, uint32_t L, StepRow* rows);

// scratch helper: grows scratch slot `i` to at least `bytes`
hipError_t scratch_get(vct_ctx* c, int i, size_t bytes, void** out);
// K4 scratch `i` (kSc*) of the ctx's current stream, grown to at least `bytes`; *fresh: it
// was (re)allocated by this call (contents undefined)
hipError_t k4_scratch(vct_ctx* c, int i, size_t bytes, void** out, bool* fresh);
// order a frame exchange (shared slot-8 / 9 scratch) after the previous one on any stream,
// and mark its end (vct_ctx::xchg_done)
hipError_t xchg_enter(vct_ctx* c);
hipError_t xchg_leave(vct_ctx* c);
// an exchange that fails after xchg_enter: record its end anyway, covering the work it
// queued on the ctx stream and the peer streams (XchgScope calls it on every early exit)
void xchg_fail(vct_ctx* c);
struct XchgScope {
    vct_ctx* c;
    bool done = false;                        // set once xchg_leave has succeeded
    ~XchgScope() { if (!done) xchg_fail(c); }
};

}  // namespace vct
