// The stencil pass of ONE tile, as TEXT: the body of k_post and of the stencil workgroups of k_post_hist (emap_kernels.hip), which
// include this file inside the kernel with POST_BX / POST_BY defined -- the tile's column in the tile grid and its tile row counted over
// the launch's row intervals (k_post: blockIdx.x / blockIdx.y; k_post_hist: derived from the linear workgroup index).  It reads the
// kernel's own parameters P, Wt, cells, trav_in, normal, plane_stride, d, S and the constants PT_R, STAGE and OUT (the output set of
// POST_CELL: POST_OUT_FULL in k_post; in k_post_hist what the frame that takes the pass along reads).
// Text and not a __device__ __forceinline__ function, for the reason POST_CELL is a macro: behind a function boundary -- parameters by
// reference or by value, with or without __restrict__, all measured -- the compiler loads the 120 filter weights of Wt once and keeps
// them live across the unrolled rows, spilling them through v_readlane / v_writelane: k_post<32, 0> 2973 -> 3589 instructions, 53 -> 56
// VGPRs, 90 -> 100 SGPRs.  Included as text the kernel's code is what it was, instruction for instruction.
// (No include guard: the file is included once per kernel.)
  int seg_b = S.b[0], seg_e = S.e[0], ty = POST_BY;
#pragma unroll
  for (int k = 1; k < 4; ++k) if (k < S.n && (int)POST_BY >= S.t0[k]) { seg_b = S.b[k]; seg_e = S.e[k]; ty = POST_BY - S.t0[k]; }
  constexpr int PT_THREADS = PT_R >= 32 ? POST_T32 : 512, PT_WAVES = PT_THREADS / 64;     // (POST_T32: compile-time knob of the A/B builds -- 256 and 1024 threads were measured slower)
  extern __shared__ float lds[];
  const int RW = PT_C + 6 + 2 * d, rp = RW + 1, RH = PT_R + 6 + 2 * d;     // staged region: tile + halo 3 + d
  const int DW = PT_C + 6, DH = PT_R + 6;                                   // region whose DILATED value is needed (halo 3)
  // Region cell (r, c) = three consecutive floats at reg[(r * rp + c) * 3]: the raw upper_bound (holes inside the DW x DH region are
  // overwritten by their dilated value), the mask >= 0 (stored as -(mask)-1 when the cell is NOT is_inside: never a source) and
  // is_valid (normal filter).  One 12-byte LDS write per staged cell; a stride of three dwords across the lanes is conflict free.
  float* reg = lds;
  int* rtab = reinterpret_cast<int*>(reg + 3 * RH * rp);       // RH + 2 row terms
  unsigned int* hs = reinterpret_cast<unsigned int*>(rtab + ((RH + 3) & ~1));      // sparse tiles: source bits of the region rows, 5 words each (post_source_masks)
  unsigned short* holes = reinterpret_cast<unsigned short*>(hs + 8 * RH);         // compacted list of the holes of the DW x DH region
  __shared__ unsigned int n_holes, s_special;
  if (threadIdx.x == 0) { n_holes = 0u; s_special = 0u; }
  __syncthreads();
  const int C = P.C;
  const int tile_r = seg_b + ty * PT_R, tile_c = POST_BX * PT_C;      // logical row / column of the tile origin
  const int tc = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // wave index in an SGPR
  // staging (post_stage_trips: rows and column walk, up to six rows' and two pairs' loads in flight per thread).  Everything that
  // depends on the row (circular origin, strip ownership, border) is computed ONCE per tile into a small LDS table.  Two forms of the walk (round 4): INTERIOR tiles need nothing else;
  // tiles along the map's edges carry the row table's and the column's flag bits (bit 31: no such cell, bit 30: border cell) and the
  // reference's flat-index row wrap (:403-407: column -1 of row r is column C - 1 of row r - 1).
  {
    const int r0 = tile_r - 3 - d, c0 = tile_c - 3 - d, EC = RW - 64;
    constexpr int U = PT_R >= 32 ? 6 : (PT_R >= 16 ? 4 : 2);                 // region rows per wave with their loads in flight together (post_stage_trips)
    // row table: region row j - 1 (one extra row on both sides for the flat-index carry) -> local row of the arrays (bits 0..23;
    // 0 with bit 31 set: not in the map / strip), bit 30: a border row (never a dilation source)
    for (int j = threadIdx.x; j < RH + 2; j += PT_THREADS) {
      const int g = r0 - 1 + j;
      const bool in_map = g >= 0 && g <= C - 1;
      const int lr = in_map ? local_row(P, phys_row(P, g)) : -1;
      const int rt = lr < 0 ? (int)0x80000000 : lr | ((g >= 1 && g <= C - 2) ? 0 : 0x40000000);
      rtab[j] = rt;
      if ((rt & (int)0xC0000000) && j >= 1 && j <= RH) s_special = 1u;      // a region row that does not exist here or is a border row (racing writers store the same value)
    }
    __syncthreads();
    // INTERIOR tiles -- every cell of the staged region exists, none is a border cell, no column leaves the map (so there is no
    // flat-index row carry): all but the tiles along the map's (or the strip's missing) edges, 82 % of the tiles at 1024^2, 98 % at
    // 8192^2.  Their staging needs none of the flag logic below: per region cell one address (row term x pitch + physical column), one
    // 16-byte load, one add, one 12-byte LDS write, one compare for the hole list -- about a dozen instructions instead of the ~85 of
    // the general path, which was 40 % of this kernel's instructions (round 4; the kernel is issue bound at every map size:
    // tools/exp_post_pitch.py).  The LDS contents are the same bit for bit.
    const bool interior = s_special == 0u && c0 >= 1 && c0 + RW - 1 <= C - 2;      // (uniform)
    auto cold_at = [&](int T, unsigned int pc) { return cells.cold[(long)(__umul24((unsigned int)T & 0xffffffu, (unsigned int)C) + pc)]; };      // row term (without its flag bits) x pitch + physical column
    if (interior) {
      const unsigned int pc0 = (unsigned int)phys_col(P, c0 + tc);
      post_stage_trips<U, PT_THREADS>(wv, tc, RH, EC, S.emagic,
        [&](int r) { return PostLd{cold_at(rtab[r + 1], pc0), 0}; },
        [&](int r, int cc) { return PostLd{cold_at(rtab[r + 1], (unsigned int)phys_col(P, c0 + cc)), 0}; },
        [&](int r, int cc, const PostLd& l) {
          const float4& q1 = l.q;
          const float m = q1.w + q1.z;
          float3 o; o.x = q1.y; o.y = m; o.z = q1.w;
          *reinterpret_cast<float3*>(reg + (r * rp + cc) * 3) = o;
          if (m < 0.5f && (unsigned int)(r - d) < (unsigned int)DH && (unsigned int)(cc - d) < (unsigned int)DW) holes[atomicAdd(&n_holes, 1u)] = (unsigned short)((r - d) * DW + (cc - d));
        });
    } else {
      // Tiles along the map's edges (or next to rows a strip does not hold): the same walk with the flag bits of the row table (bit 31:
      // no such row, bit 30: border row) and of the column (the same two bits + the flat-index row carry dr of the reference's
      // addressing, :403-407: column -1 of row r is column C - 1 of row r - 1 -- such a lane reads the row table one row up or down).
      // A cell that does not exist loads cell (0, 0) of the arrays and is masked afterwards: no branch around the loads.
      auto col_terms = [&](int cc, int& dr, int& pc, int& flags) {     // region column -> row carry, physical column, flag bits
        int cl = c0 + cc; dr = 0;
        if (cl < 0) { cl += C; dr = -1; } else if (cl >= C) { cl -= C; dr = 1; }
        flags = ((cl >= 1 && cl <= C - 2) ? 0 : 0x40000000) | (cl < C ? 0 : (int)0x80000000);      // (a region wider than the map: columns past the wrap are unused)
        pc = cl < C ? phys_col(P, cl) : 0;
      };
      int ldr, lpc, lfl;
      col_terms(tc, ldr, lpc, lfl);
      const int* ltab = rtab + 1 + ldr;                              // the lane's view of the row table
      post_stage_trips<U, PT_THREADS>(wv, tc, RH, EC, S.emagic,
        [&](int r) { const int T = ltab[r]; return PostLd{cold_at(T, (unsigned int)lpc), T | lfl}; },
        [&](int r, int cc) {
          int dr, pc, fl;
          col_terms(cc, dr, pc, fl);
          const int T = rtab[r + 1 + dr];
          return PostLd{cold_at(T, (unsigned int)pc), T | fl};
        },
        [&](int r, int cc, const PostLd& l) {
          const float4& q1 = l.q;
          const bool ok = l.tag >= 0, inside = (l.tag & 0x40000000) == 0;
          const float m = q1.w + q1.z;
          float3 o;
          o.x = ok ? q1.y : 0.f;
          o.y = ok ? (inside ? m : -m - 1.f) : -1.f;                  // mask >= 0; stored as -(mask) - 1 when the cell is not is_inside: never a source
          o.z = ok ? q1.w : 0.f;
          *reinterpret_cast<float3*>(reg + (r * rp + cc) * 3) = o;
          // a hole of the region whose dilated value is needed (cells outside the map are never sources and never outputs: not listed)
          if (ok && m < 0.5f && (unsigned int)(r - d) < (unsigned int)DH && (unsigned int)(cc - d) < (unsigned int)DW) holes[atomicAdd(&n_holes, 1u)] = (unsigned short)((r - d) * DW + (cc - d));
        });
    }
  }
  // The holes of the DW x DH region were COMPACTED into an LDS list by the staging loop and are searched one hole per lane -- a
  // hole-containing wave would otherwise drag all 64 lanes through the neighbour search (measured: 11 of 33 us with 1.5 % holes), and
  // a separate detection pass over the region with its two barriers cost 5.8 us of a 23-us kernel even when there was no hole at all.
  // The dilated value replaces the raw one IN PLACE: only cells with mask > 0.5 are ever sources and the masks are not touched, so a
  // filled hole cannot feed another hole (Jacobi semantics of the reference kernel), and the stencils below read one array.
  __syncthreads();
  const unsigned int nh = n_holes;
  const bool sparse = 4 * (int)nh > 3 * DW * DH && RW <= 128 && d <= 15;       // (uniform) three cells of four are holes
  if (sparse) {                                                     // mostly unknown tile: the search on bit masks (post_first_source)
    post_source_masks<PT_THREADS>(hs, RH, RW, [&](int r, int cc) { return reg[(r * rp + min(cc, RW - 1)) * 3 + 1] > 0.5f; });
    for (unsigned int hi = threadIdx.x; hi < nh; hi += PT_THREADS) {
      const int pos = holes[hi], r = pos / DW, cc = pos - r * DW;
      int dy, dx;
      if (!post_first_source(hs, r + d, cc + d, d, dy, dx)) continue;      // no source within reach: the raw value stays
      const int o0 = (r + d) * rp + (cc + d);
      reg[o0 * 3] = reg[(o0 + dy * rp + dx) * 3];                    // a hole's slot is never read by another search (its mask is < 0.5)
    }
  } else
  for (unsigned int hi = threadIdx.x; hi < nh; hi += PT_THREADS) {
    const int pos = holes[hi], r = pos / DW, cc = pos - r * DW;
    const int o0 = (r + d) * rp + (cc + d);
    // first hit on ascending anti-diagonals == the reference's scan order with its signed dx+dy criterion (:429-436)
    bool found = false;
    for (int s2 = -2 * d; s2 <= 2 * d && !found; ++s2) {
      const int dy0 = max(-d, s2 - d), dy1 = min(d, s2 + d);
      for (int dy = dy0; dy <= dy1; ++dy) {
        const int o = o0 + dy * rp + (s2 - dy);
        if (reg[o * 3 + 1] > 0.5f) { reg[o0 * 3] = reg[o * 3]; found = true; break; }     // a hole's slot is never read by another search (its mask is < 0.5)
      }
    }
  }
  if (nh) __syncthreads();                       // (uniform: every thread read the same count)
  const int col = tile_c + tc;                   // logical column
  if (col >= C) return;
  const int pcol = phys_col(P, col);
  const float* dil = reg + (d * rp + d) * 3;     // dilated plane of the DW x DH region: element (row, column) at (row * dp + column) * 3
  const int dp = rp;
  // Every wave owns PT_R / 8 consecutive tile rows of its column.  The four channels of a dilated 3x3 filter go through packed
  // fp32 FMAs in PAIRS (v_pk_fma_f32: the two channels' weights are one aligned scalar register pair, the tap is broadcast): each
  // channel keeps the reference's tap order, and the 1x1 output convolution is the same scalar chain over (filter, channel) as the
  // unfused stage -- half the vector instructions of the 12 x 9-tap filter bank, identical sums.
  constexpr int RPW = PT_R >= PT_WAVES ? PT_R / PT_WAVES : 1;
  const bool col_in = STAGE == 0 && col >= 3 && col <= C - 4;
  const bool col_n = col >= 1 && col <= C - 3;
#pragma unroll
  for (int k = 0; k < RPW; ++k) {
    const int tr = wv * RPW + k, gr = tile_r + tr;                 // scalar
    if (tr >= PT_R || gr >= seg_e) break;
    const float* t0 = &dil[((tr + 3) * dp + (tc + 3)) * 3];
    const long c = (long)(rtab[tr + 4 + d] & 0xffffff) * C + pcol;
    POST_CELL(Wt, 3, t0, dp, t0[2], col_in && gr >= 3 && gr <= C - 4, col_n && gr >= 1 && gr <= C - 3, c);
  }
