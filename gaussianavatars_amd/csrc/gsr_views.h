// gsr_views.h -- host only: the arithmetic the state-buffer layouts and the launches share, and typed views of the three state
// buffers of include/gsr.h (geometry, binning, image).  make_views is the one place where a layout offset becomes a pointer;
// gsr_api.hip's forward and backward launch through what it returns.
#pragma once

#include "gsr_device.h"

namespace gsr_host {

struct TileGrid { int gx, gy; size_t tiles; };
inline TileGrid tile_grid(int W, int H)
{
    const int gx = (W + GSR_BLOCK_X - 1) / GSR_BLOCK_X, gy = (H + GSR_BLOCK_Y - 1) / GSR_BLOCK_Y;
    return {gx, gy, (size_t)gx * (size_t)gy};
}
// the reference-format key / point lists are materialised (the parity modes; production -- 1, 3, 4, 6 -- does not write them)
inline bool reference_lists(int32_t tile_culling) { return tile_culling == 0 || tile_culling == 2; }
constexpr size_t splat_blocks(size_t P) { return (P + 255) / 256; }   // k_preprocess's workgroups
// GsrBinningLayout.pstat (rank path): one uint4 row of statistics per k_preprocess workgroup, four planes [workgroups] of uint4 group sums,
// then k_rcount's chunk boundaries, one per rank workgroup and the end (gsr_device.h: PreprocessArgs.pstat, rank_map)
constexpr size_t pstat_bytes(size_t pblocks) { return pblocks * 5 * sizeof(uint4) + (GSR_RANK_BLOCKS + 4) * 4; }
inline uint32_t* pstat_chunk_bounds(uint4* pstat, size_t pblocks) { return reinterpret_cast<uint32_t*>(pstat + 5 * pblocks); }

// ---- the views: every field as the pointer the kernels take; nullptr where this frame's binning path or mode does not have the
// field and the launches pass nullptr.  The backward, which only reads the binning and image states, takes them as const views.
struct GeomView {   // GsrGeomLayout
    float* depths; float4* grec; float* cov3D; ushort4* rect; uint32_t* tiles_touched; uint8_t* clamped; uint8_t* visible;
    float4* brec;                 // depth-ordered scatter only
    float4* acc64; float4* acc;   // the forward zeroes them as float4 records; the backward sums into them as:
    float* acc_sums() const { return reinterpret_cast<float*>(acc); }               // [P][12] floats
    long long* acc64_sums() const { return reinterpret_cast<long long*>(acc64); }   // [P][10] fixed-point sums (deterministic mode)
    float* shjac;
};
struct BinView {    // GsrBinningLayout
    gsr::BinHeader* hdr; unsigned long long* total; unsigned long long* rect_total;   // the header; its words 0 and 1
    unsigned long long* keys; uint32_t* qlist;   // reference_lists only
    uint32_t *point_list, *qpos, *qcount, *qstart, *tile_count, *tile_start, *tile_cursor, *tile_order, *block_hist;
    uint2* ranges; uint4* tdesc;
    unsigned long long *dkeys, *dtmp, *qmask;
    uint32_t *order, *bcount, *bstart, *bcursor, *border, *bhist, *qhist, *qprefix;
    uint2* ranks; uint32_t* rank; uint32_t* rank_over; uint32_t* bandcnt;
    uint2* obs;                                  // more than one band only
    ushort4* srect; float4* sspan;
    uint4* pstat; uint32_t* chunk_bounds;        // rank path only
};
struct ImageView {  // GsrImageLayout
    float* final_T; uint32_t *n_contrib, *n_contrib_q; float* c_final; float4* ck; uint32_t *gmax, *units;
};
struct StateViews {
    GsrBinningLayout bl;   // path, nb, chunks, nbands, band_rows
    TileGrid tg;
    GeomView g; BinView b; ImageView im;
};

template <class T> T* at(void* base, size_t offset) { return reinterpret_cast<T*>(static_cast<char*>(base) + offset); }

// The three layouts of a frame (its arguments are checked by then: the layout calls cannot fail) and the views of its buffers
inline void make_views(int32_t P, int W, int H, int64_t capacity, int32_t tile_culling, void* geom, void* binning, void* img, StateViews* v)
{
    GsrGeomLayout gl;
    GsrBinningLayout& bl = v->bl;
    GsrImageLayout il;
    gsr_geom_layout(P, &gl);
    gsr_binning_layout(capacity, W, H, P, tile_culling, &bl);
    gsr_image_layout(W, H, &il);
    v->tg = tile_grid(W, H);
    const bool prod = bl.path == 1, rankp = bl.path == 0, lists = reference_lists(tile_culling);
    GeomView& g = v->g;
    g.depths = at<float>(geom, gl.depths);                g.grec = at<float4>(geom, gl.grec);
    g.cov3D = at<float>(geom, gl.cov3D);                  g.rect = at<ushort4>(geom, gl.rect);
    g.tiles_touched = at<uint32_t>(geom, gl.tiles_touched);
    g.clamped = at<uint8_t>(geom, gl.clamped);            g.visible = at<uint8_t>(geom, gl.visible);
    g.brec = prod ? at<float4>(geom, gl.brec) : nullptr;
    g.acc64 = at<float4>(geom, gl.acc64);                 g.acc = at<float4>(geom, gl.acc);
    g.shjac = at<float>(geom, gl.shjac);
    BinView& b = v->b;
    b.hdr = at<gsr::BinHeader>(binning, 0);
    b.total = &b.hdr->total;                              b.rect_total = &b.hdr->rect_total;
    b.keys = lists ? at<unsigned long long>(binning, bl.keys) : nullptr;
    b.qlist = lists ? at<uint32_t>(binning, bl.qlist) : nullptr;
    b.point_list = at<uint32_t>(binning, bl.point_list);  b.qpos = at<uint32_t>(binning, bl.qpos);
    b.qcount = at<uint32_t>(binning, bl.qcount);          b.qstart = at<uint32_t>(binning, bl.qstart);
    b.tile_count = at<uint32_t>(binning, bl.tile_count);  b.tile_start = at<uint32_t>(binning, bl.tile_start);
    b.tile_cursor = at<uint32_t>(binning, bl.tile_cursor); b.tile_order = at<uint32_t>(binning, bl.tile_order);
    b.block_hist = at<uint32_t>(binning, bl.block_hist);
    b.ranges = at<uint2>(binning, bl.ranges);             b.tdesc = at<uint4>(binning, bl.tdesc);
    b.dkeys = at<unsigned long long>(binning, bl.dkeys);  b.dtmp = at<unsigned long long>(binning, bl.dtmp);
    b.qmask = at<unsigned long long>(binning, bl.qmask);  b.order = at<uint32_t>(binning, bl.order);
    b.bcount = at<uint32_t>(binning, bl.bcount);          b.bstart = at<uint32_t>(binning, bl.bstart);
    b.bcursor = at<uint32_t>(binning, bl.bcursor);        b.border = at<uint32_t>(binning, bl.border);
    b.bhist = at<uint32_t>(binning, bl.bhist);
    b.qhist = at<uint32_t>(binning, bl.qhist);            b.qprefix = at<uint32_t>(binning, bl.qprefix);
    b.ranks = at<uint2>(binning, bl.ranks);               b.rank = at<uint32_t>(binning, bl.rank);
    b.rank_over = at<uint32_t>(binning, bl.rank_over);    b.bandcnt = at<uint32_t>(binning, bl.bandcnt);
    b.obs = bl.nbands > 1 ? at<uint2>(binning, bl.obs) : nullptr;
    b.srect = at<ushort4>(binning, bl.srect);             b.sspan = at<float4>(binning, bl.sspan);
    b.pstat = rankp ? at<uint4>(binning, bl.pstat) : nullptr;
    b.chunk_bounds = rankp ? pstat_chunk_bounds(b.pstat, splat_blocks((size_t)P)) : nullptr;
    ImageView& im = v->im;
    im.final_T = at<float>(img, il.final_T);              im.n_contrib = at<uint32_t>(img, il.n_contrib);
    im.n_contrib_q = at<uint32_t>(img, il.n_contrib_q);   im.c_final = at<float>(img, il.c_final);
    im.ck = at<float4>(img, il.ck);                       im.gmax = at<uint32_t>(img, il.gmax);
    im.units = at<uint32_t>(img, il.units);
}

}  // namespace gsr_host
