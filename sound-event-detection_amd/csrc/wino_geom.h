// Item geometry of the two Winograd conv kernels (conv_wino.hip,
// conv_wino43.hip): what a workgroup covers and how its LDS is laid out.
// Plain constexpr structs and no HIP header, so the kernels and the host's
// launch plan (plan.cpp) read the same numbers.
#pragma once

namespace sedx {

// ---- F(2x2,3x3), conv_wino.hip -----------------------------------------------
// TG tile groups (32 tiles each) x 32 NT channels per workgroup, 4 TG waves.
// C1 (block 1, F = 64): the input is the bn0 output X0 [B][T][64] and conv1
// (Cin 1 -> 64, BN folded, ReLU) is computed into each chunk's halo image in
// LDS (below): conv1's 64-channel activation never exists in HBM.
template <int F, int TG, int NT = 2, bool C1 = false>
struct WinoGeom {
  static constexpr int WAVES = 4 * TG;               // row waves 0..3 of each tile group
  static constexpr int THREADS = 64 * WAVES;
  static constexpr int NCH = 32 * NT;                // output channels per workgroup
  static constexpr int P = 32 * TG;                  // tiles per workgroup
  static constexpr int FT = F / 2;                   // tiles per tile row
  static constexpr int TRW = P / FT;                 // tile rows per workgroup
  static constexpr int RT = 2 * TRW + 2, CS = F + 2, KC = 4;
  static constexpr int PL = RT * CS;                 // halo pixels
  static constexpr int PLP = (PL + 63) / 64 * 64;    // whole 64-pixel DMA units
  // floats: [pixel][4 ch] (C1: a 64-pixel conv1 group for every wave; the
  // groups past the halo write zeros into the padding)
  static constexpr int A_SZ = KC * (C1 && PLP < 64 * WAVES ? 64 * WAVES : PLP);
  static constexpr int W_SZ = 16 * KC * NCH;         // floats: [p][h][n NCH][ks]
  static constexpr int BUF = A_SZ + W_SZ;
#ifndef SEDX_WINO_NBUF
#define SEDX_WINO_NBUF 3
#endif
  static constexpr int NBUF = SEDX_WINO_NBUF;        // ring depth
  static constexpr int UW = W_SZ / 256;              // 1-KiB DMA units per chunk
  static constexpr int UA = C1 ? 0 : PLP / 64;       // halo units (C1 computes the halo instead)
  static constexpr int U = UW + UA;
  static constexpr int UPW = (U + WAVES - 1) / WAVES;
  static constexpr int VM_MIN = U / WAVES;           // units of the wave with the fewest
  // epilogue exchange, one channel tile per round: per tile group
  // [finisher row 4][other row 3][register 4][z 2][lane 64] floats
  static constexpr int XTG = 4 * 3 * 4 * 2 * 64;
  static constexpr int XCH = TG * XTG;
  // C1: an item's X0 rows t0 - 2 .. t0 + RT - 1 ([row][F], zero rows outside
  // the clip), two buffers by item parity, in 1-KiB DMA units; the conv1
  // halo pixels in 64-pixel groups, one group per wave
  static constexpr int XROWS = RT + 2;
  static constexpr int UX = C1 ? (XROWS * F + 255) / 256 : 0;
  static constexpr int X0_SZ = 256 * UX;
  static constexpr int XA_OFF = NBUF * BUF + XCH;
  // the layer's biases (Cout <= 512), LDS-DMA'd once in the prologue: read
  // from LDS, the epilogue's bias needs no vmcnt wait (which would also wait
  // for the next item's DMAs in flight)
  static constexpr int BIAS_OFF = XA_OFF + 2 * X0_SZ, BIAS_MAX = 512;
  // C1 with conv1 on the matrix pipe: conv1's weights [64 ch][9] (3 DMA
  // units, zero-padded) and biases (1 unit), LDS-DMA'd in the prologue
  static constexpr int W1_OFF = BIAS_OFF + BIAS_MAX, W1_SZ = C1 ? 1024 : 0;
  static constexpr int LDS_BYTES = 4 * (W1_OFF + W1_SZ);   // ring, epilogue exchange, X0 tiles, biases, conv1 weights
  static constexpr int WG_PER_CU = WAVES == 8 || LDS_BYTES > 80 * 1024 ? 1 : 2;
  static_assert(NT == 1 || NT == 2, "channel tiles per wave");
  static_assert(P % FT == 0, "whole tile rows per workgroup");
  static_assert(VM_MIN * (NBUF - 1) <= 63, "vmcnt field");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS per workgroup");
  static_assert(!C1 || (F == 64 && NT == 2 && PLP <= 64 * WAVES && UX <= WAVES && NBUF >= 3), "C1: block 1 (64 bins), a conv1 group per wave");
};

// ---- F(4x4,3x3), conv_wino43.hip ---------------------------------------------
#ifndef SEDX_W43_EPI2
#define SEDX_W43_EPI2 0
#endif
// Item claims (SEDX_W43_CLAIM 1, the default; launches with more items than
// CUs): a persistent grid, one workgroup per CU, whose workgroups claim their
// items from the counter of their XCD lane x = blockIdx & 7 (items 8 v + x,
// the static decode's XCD mapping), so a workgroup that starts late — its CU
// held by the other batch's GRU — takes fewer items instead of costing a
// whole extra round.  The first two items come in one claim at the top; the
// item after next is claimed at an item's epilogue by its last wave (not a
// finisher) and lands in LDS before the epilogue's last round, read by every
// wave at the next item's top.  Counters (sched): 8 ints 128 B apart + a
// done count at [255], zero at launch; the last workgroup to finish zeroes
// them again.  0: the static grid-stride order of round 5 (A/B builds).
#ifndef SEDX_W43_CLAIM
#define SEDX_W43_CLAIM 1
#endif

// TG: tile groups per item — 2 (32 tiles, 12 waves; every full-size launch)
// or 1 (16 tiles, 6 waves: the one-clip grids of the 16-channel items at
// F = 16 / 8, twice the items of 2 for the same work)
// PL (block 1's conv2, F = 64 only): the input is channel-planar
// [B][64][T][64] (conv1_planar_kernel), so a halo row of a plane is 64
// contiguous floats and the halo is staged by 16-byte LDS-DMAs, four pixels
// per lane: one 1-KiB piece per wave per step (wave w: third w % 3 of plane
// w / 3) instead of four 256-byte planes.  The output layout is unchanged.
template <int F, int TG = 2, bool PL = false>
struct W43Geom {
  static constexpr int WAVES = 6 * TG, THREADS = 64 * WAVES;
  static constexpr int NT = 4, NCH = 64;             // channel tiles / output channels per item
  static constexpr int TILES = 16 * TG;              // TG tile groups of 16
  static constexpr int FT = F / 4;                   // tiles per tile row
  static constexpr int TRW = TILES / FT;             // tile rows per item
  // a tile group is TRG tile rows x TFG tile columns (lane n = tr TFG + tf)
  static constexpr int TFG = F == 8 ? 2 : F == 64 ? 16 : 4;
  static constexpr int TRG = 16 / TFG;
  static constexpr int RT = 4 * TRW + 2, CS = F + 2; // halo rows / columns
  // halo row stride: (4 tr RS + 4 tf) / 2 over the 16 tiles of a group must
  // take the 16 even values mod 32 (b64 bank pairs): 2 RS = 8 (mod 32) for
  // 4 x 4 groups, 2 RS = 20 (mod 32) for 8 x 2
  // (F = 64, block 1: one tile row of 16 per group, 2 tf = 0, 2, .., 30 for any even RS)
  // PL: a row image is [4 zero][64 pixels][4 zero] — 18 groups of 4 dwords,
  // groups 0 and 17 zero-filled by the DMA's range check — written one dword
  // into the plane (M0 + 4 bytes: measured fine for 16-byte LDS-DMAs,
  // tools/oob_lds_probe.cpp), so column -1 is index 4 and column 64 index 69:
  // a patch starts on an even dword.  (At index 3 the patch reads were
  // ds_read_b64 at odd dwords — correct, and 17 times slower in that probe.)
  static constexpr int RS = PL ? 72 : F == 64 ? 66 : F == 32 ? 36 : F == 16 ? 20 : 10;
  // a plane's halo in 64-dword DMA blocks, one per wave 0..HB-1 (RT RS <= 704
  // for every F); wave 11 issues its four halo DMAs into an LDS trash block,
  // so every wave has the same DMA count per step (TG 1: RT RS <= 384, a
  // block per wave, no trash wave)
  static constexpr int HB = TG == 2 ? 11 : 6;
  // PL: a plane is dword 0 (never read), then three 256-dword pieces (RT RS
  // = 720 dwords of rows, the rest zero-filled)
  static constexpr int PS = PL ? 3 * 256 + 2 : 64 * HB + 2;   // plane stride, = 2 mod 4 (odd bank pairs for odd k)
  static constexpr int HALO = 4 * PS;                // dwords per halo slot
  static constexpr int USZ1 = 36 * 4 * 16;           // NT 1: one 16-channel tile's slab ([p][k][m]), 9 KiB
  static constexpr int NB = 3;                       // ring depth (U and halo)
  // epilogue exchange per round, per tile group, in the U slot freed by the
  // item's last step: STORE [row 6][reg 2][kc 4][16 tiles + 4 pad][4 z] (the
  // pad: a finisher's reads of 4 kc x 16 consecutive (tile, column) words
  // hit 64 banks), else [row 6][reg 2][z pair 2][lane 64][2] (a finisher's
  // ds_read_b64 of its own pair: conflict-free)
  static constexpr int XRS = 4 * 80;
  static constexpr int XTG = 6 * 2 * XRS;
  // dwords per U slot: the 64-channel slab ([p][k][m][nt]); TG 1 (NT 1 only):
  // its 9 KiB slab or one tile group's exchange, the larger
  static constexpr int USZ = TG == 2 ? 36 * 4 * NCH : (USZ1 > XTG ? USZ1 : XTG);
  static constexpr int U_OFF = 0, H_OFF = NB * USZ, BIAS_OFF = H_OFF + NB * HALO, BIAS_MAX = 512;
  static constexpr int HTRASH_OFF = BIAS_OFF + BIAS_MAX;   // 64 dwords: wave 11's halo DMAs
  // a second exchange area (SEDX_W43_EPI2, pooled / freq-mean epilogues): one
  // tile group's [row 6][reg 2][z pair 2][lane 64][2] for registers 2, 3
  static constexpr int X2_OFF = HTRASH_OFF + 64, X2 = SEDX_W43_EPI2 && TG == 2 ? 3072 : 0;
  static constexpr int CL_OFF = X2_OFF + X2;         // item claims: the landed claim ([0]) and the first item ([1])
  static constexpr int LDS_BYTES = 4 * (CL_OFF + (SEDX_W43_CLAIM ? 4 : 0));
  static constexpr int VM = PL ? 4 : 7;              // DMAs per wave per step (3 U units + 4 halo planes; PL: + 1 piece)

  static_assert(F == 64 || F == 32 || F == 16 || F == 8, "F");
  static_assert(PL ? RT * RS <= 3 * 256 && 1 + 3 * 256 <= PS : RT * RS <= 64 * HB, "halo plane fits its DMA blocks");
  static_assert(!PL || (F == 64 && TG == 2 && WAVES == 12 && RS == 4 * 18), "planar input: block 1, four planes x three pieces");
  static_assert(PS % 4 == 2 && PS >= RT * RS, "plane stride");
  static_assert(TG == 1 || TG == 2, "TG");
  static_assert(TG == 1 ? HB == WAVES : HB == WAVES - 1, "halo blocks: one per wave (TG 2: wave 11 trash)");
  static_assert(TG == 1 || 36 % WAVES == 0, "U units per wave");
  static_assert(TG * XTG <= USZ, "the tile groups' exchange fits one U slot");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS per workgroup");
  static_assert(FT * TRW == TILES && TFG * TRG == 16, "tile groups");
};

}  // namespace sedx
