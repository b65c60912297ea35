// pfr_tilewalk.h — the tile queue of the pair entry points, in ONE place: persistent workgroups walk a queue of 128 x 128 tiles in
// super-tiles of 16 x 16 tiles (what the chip works on at any time is a few MB of rows).  Queue index t = super-tile * 256 + tile inside;
// super-tiles are row-major, tiles inside a super-tile are row-major.  Symmetric mode enumerates the super-tiles of the upper triangle
// only and skips the tiles below the diagonal; slots past the last tile row / column are skipped in both modes.  The decode is plain
// integer / double arithmetic for host and device (pfr_pair_tile_coords runs it on the host); the geometry and the grid size are the
// host side of the same walk.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define TW_FN __host__ __device__ __forceinline__
#else
#define TW_FN inline
#endif

#define RC_T 128            // tile rows / columns
#define RC_SUPER 16         // super-tile edge in tiles

struct TileWalk {
  int ntm, ntn, nsn;        // tiles per dimension, super-tiles per row of super-tiles
  long long nsuper;         // super-tiles in the queue: t runs over [0, nsuper * RC_SUPER * RC_SUPER)
};

// super-tile su -> (sm, sn)
TW_FN void tw_super(long long su, int nsn, int sym, int& sm, int& sn) {
  if (sym) {
    // super-tile su of the upper triangle, row-major: row r starts at r * ns - r (r - 1) / 2
    const double ns2 = 2.0 * nsn + 1.0;
    int r = (int)((ns2 - sqrt(ns2 * ns2 - 8.0 * (double)su)) * 0.5);
    r = r < 0 ? 0 : (r > nsn - 1 ? nsn - 1 : r);
    while (r > 0 && (long long)r * nsn - (long long)r * (r - 1) / 2 > su) --r;
    while ((long long)(r + 1) * nsn - (long long)(r + 1) * r / 2 <= su) ++r;
    sm = r;
    sn = r + (int)(su - ((long long)r * nsn - (long long)r * (r - 1) / 2));
  } else {
    sm = (int)(su / nsn);
    sn = (int)(su % nsn);
  }
}

// queue index t -> (tm, tn); false: the slot holds no tile (past ntm / ntn, or below the diagonal in symmetric mode)
TW_FN bool tw_tile(long long t, int ntm, int ntn, int nsn, int sym, int& tm, int& tn) {
  const long long su = t / (RC_SUPER * RC_SUPER);
  const int l = (int)(t % (RC_SUPER * RC_SUPER));
  int sm, sn;
  tw_super(su, nsn, sym, sm, sn);
  tm = sm * RC_SUPER + l / RC_SUPER;
  tn = sn * RC_SUPER + l % RC_SUPER;
  return !(tm >= ntm || tn >= ntn || (sym && tn < tm));
}

// ---- host side: the geometry of a walk over ntm x ntn tiles (symmetric: ntm == ntn) and its grid
static inline TileWalk tw_from_tiles(int ntm, int ntn, bool sym) {
  TileWalk w;
  w.ntm = ntm; w.ntn = ntn;
  w.nsn = (ntn + RC_SUPER - 1) / RC_SUPER;
  const int nsm = (ntm + RC_SUPER - 1) / RC_SUPER;
  w.nsuper = sym ? (long long)w.nsn * (w.nsn + 1) / 2 : (long long)nsm * w.nsn;
  return w;
}

static inline TileWalk tw_from_rows(int Na, int Nb, bool sym) {
  return tw_from_tiles((int)(((long long)Na + RC_T - 1) / RC_T), (int)(((long long)Nb + RC_T - 1) / RC_T), sym);
}

static inline long long tw_ntiles(const TileWalk& w, bool sym) {
  return sym ? (long long)w.ntn * (w.ntn + 1) / 2 : (long long)w.ntm * w.ntn;
}

// persistent workgroups: wg_per_cu per compute unit, never more than there are tiles
static inline unsigned tw_grid(long long ntiles, int wg_per_cu, int cus) {
  const long long wgs = (long long)wg_per_cu * cus;
  return (unsigned)(ntiles < wgs ? ntiles : wgs);
}
