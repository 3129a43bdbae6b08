#!/usr/bin/env python3
"""Generator of the K loop of gemm_g4 (csrc/gemm_g4.hip): writes gemm_g4_body.inc -- ONE asm statement that takes a 256 x 256 output
tile from "nothing staged" to "accumulators complete" --, gemm_g4_sk_sum.inc (the split-K sum) and gemm_g4_regs.h (register
constraints, clobbers and LDS map).  Run by build.py when stale; the outputs are committed.

Shape of the kernel: four waves (2 x 2), ONE per SIMD, 128 x 128 wave tiles (256 accumulator registers in the AGPR half of the file),
K-tiles of 64 16-bit elements = 128-byte LDS rows, operands by LDS-DMA into [A0 | A1 | A2 | W0 | W1] x 32 KiB (256 rows each).  A wave
tile of 128 x 128 reads 8 fragments per 16 MFMA where the eight-wave 128 x 64 tiling of gemm_bf16_pp64 reads 12, and with one wave per
SIMD nothing arbitrates: the stream below IS the schedule.  Per K-tile and wave: 64 MFMA (2065 matrix-pipe cycles), 32 ds_read_b128,
16 LDS-DMA pieces + 16 M0 writes, 4 v_add_u32 and 9 SALU of pointer and stage arithmetic, ONE barrier.
The 16-bit element type is not in the body: the MFMA lines end in the string macro G4_T16 ("bf16" or "f16"), which gemm_g4.hip defines
around each #include -- staging, swizzle and fragment reads move 16-bit elements whatever they encode.
Why asm (as attention_q4): with more than 256 registers hipcc selects AGPR-form MFMAs and moves operands through v_accvgpr copies, puts
s_nop / s_waitcnt where its hazard model wants them and the 64-bit-vaddr form of the LDS-DMA inside loops; the round-2 C++ kernel of
this shape (gemm_q4, diagnostics library) ran 2300-2500 cycles per K-tile.

Schedule of K-tile t (g = t & 1: W stage and fragment-address register set; the A stage is run-time state), four steps s of 16 MFMA
(acc[i][j] += W-fragment i x A-fragment j of k-step s):
  every step : first 8 MFMA slots carry the 8 fragment reads of the NEXT step (step 3: of step 0 of K-tile t+1)
  step 0     : A pieces of K-tile t+2 -> A stage (t+2) % 3 (LDS offset s43; free since the barrier of K-tile t-1), one per two MFMAs
  step 1     : A fragment addresses of K-tile t+1 (set g^1, idle since step 3 of K-tile t-1) = s42 + stage-0 addresses v[100:103]; then
               rotate: s42 <- s43, s43 <- (s43 + 32 KiB) mod 96 KiB
  step 3     : s_waitcnt vmcnt(8) lgkmcnt(0) + s_barrier first, then W pieces of K-tile t+2 -> W stage g (free since that barrier)
vmcnt counts in issue order, so an operand only gains lead if what is issued BEHIND it may stay in flight at the wait: at vmcnt(8) K-tile
t+1 has landed and the A pieces of K-tile t+2 are still on their way.  A -- the operand that streams from HBM (FF2: 0.94 GB; the weights
come back from the MALL) -- has 1.75 K-tiles to arrive, W 1.0.
RAW: every wave's vmcnt(8) precedes the barrier of step 3 of K-tile t; the first read of K-tile t+1 is that step's fragment read.  WAR:
the last reads of W stage g are the fragment reads of step 2 of K-tile t, those of A stage (t+2) % 3 = (t-1) % 3 belong to K-tile t-1; both
completed (lgkmcnt(0)) before the barrier that precedes the overwriting DMA.
Measured (tools/stall_g4.py, tools/g4_ablate.sh; cycles per K-tile, floor 2065): without the LDS-DMA instructions the loop runs AT the
floor (2063.5) with every read, wait and barrier in place -- all overhead is DMA, its issue cost or its latency; this schedule runs
QKV 2130, out 2177, FF1 2158, FF2 2141 (profiles/r04_gemm_g4_a3.txt).  Rejected, each built and measured (HISTORY.md, GEMM and section 12):
  * two stages [A | W] x 64 KiB, W pieces in step 0 and A pieces in step 3: 2153 / 2267 / 2193 / 2439 (profiles/r04_gemm_g4_a3.txt)
  * all 16 pieces right behind the barrier: 2770 -- back-to-back LDS-DMA stalls the issuing wave, pieces must be SPREAD (HISTORY.md)
  * a ring of five K32 stages, pieces four tiles ahead: 2410-2750 (HISTORY.md)
  * an L2 prefetch by two global_load_dword per wave and K-tile: 2470-3070 (HISTORY.md)
  * register-staged operands (global_load_dwordx4 two K-tiles ahead, ds_write_b128): 2340-2480 against 2154-2453 (HISTORY.md)
  * three W stages instead of three A stages: level with two stages, 2152 / 2282 / 2188 / 2459 (profiles/r03_gemm_g4_w3.txt)
  * nt on the A / W pieces: QKV 2368 / 2243 against 2152; sc1, sc0 sc1: level (profiles/r04_gemm_g4_cache_policy.txt)
Registers: a[0:255] acc[i][j] at 64 i + 16 j (OUT); v[0:63] fragments [buffer][W 0-3 | A 0-3]; v[64:79] IN fragment addresses
[A | W][parity][step]; v[80:95] IN staging offsets [A | W][piece]; v[96:97] IN unused (see main()); v98 IN lane * 16 (split K);
v[100:103] stage-0 A fragment addresses; s[36:37] / s[38:39] IN next A / W K-tile to stage; s40 IN LDS address of the wave's piece 0 of A
in stage 0; s41 IN number of [odd, even] K-tile pairs of the loop = (nT - 4) / 2; s42 / s43 / s48 A stage rotation; s[44:47] IN split K;
nT = K / 64 even, >= 4.
"""
import os

from asmgen import ablations, ar, define_clobbers, define_regs, drops_opcodes, emitter, frag_read, lds_dma, m0_piece, out_dir, ptr_advance, vr, write_inc

FRAG, VADDR, VOFF, ABASE = 0, 64, 80, 100
S_A, S_W, S_M0W, S_CNT, S_ANEXT, S_ADMA, S_AM0 = 36, 38, 40, 41, 42, 43, 48
A_STRIDE, W_BASE, W_STRIDE, LDS_BYTES = 32768, 98304, 32768, 163840
ABLATE = ablations("G4_ABLATE")
DROPS = {"nodma": ["global_load_lds_dwordx4"], "noread": ["ds_read_b128"], "nobar": ["s_barrier"]}
MFMA = 'v_mfma_f32_32x32x16_" G4_T16 "'  # closes and reopens the string literal of the line: gemm_g4.hip defines G4_T16 as "bf16" or "f16"


def wf(buf, i):
    return FRAG + 32 * buf + 4 * i


def af(buf, j):
    return FRAG + 32 * buf + 16 + 4 * j


def vaddr(is_w, g, s):
    return VADDR + (8 if is_w else 0) + 4 * g + s


def frag(buf, n, g, s):
    """fragment n (0-3 W, 4-7 A) of step s of the K-tile whose fragment-address set is g -> buffer buf"""
    return frag_read(wf(buf, n) if n < 4 else af(buf, n - 4), vaddr(n < 4, g, s), n)


def ktile(emit, g, first=False, dma=True, last=False):
    """K-tile t (parity g); dma: it stages K-tile t+2"""
    for s in range(4):
        cur, nxt = s & 1, (s & 1) ^ 1
        if s == 3 and not last:
            emit(f"s_waitcnt vmcnt({8 if dma else 0}) lgkmcnt(0)", "s_barrier")
        else:
            emit("s_waitcnt lgkmcnt(0)")
        if s == 0 and dma:
            emit(f"s_add_u32 s{S_AM0}, s{S_M0W}, s{S_ADMA}")
        for k in range(16):
            i, j = k >> 2, k & 3
            acc = ar(64 * i + 16 * j, 16)
            emit(f"{MFMA} {acc}, {vr(wf(cur, i), 4)}, {vr(af(cur, j), 4)}, {'0' if (first and s == 0) else acc}")
            if k < 8 and not (last and s == 3):
                emit(frag(nxt, k, g, s + 1) if s < 3 else frag(nxt, k, g ^ 1, 0))
            p = k >> 1
            if s == 0 and dma:  # A piece p of K-tile t+2 -> A stage (t+2) % 3
                emit(m0_piece(S_AM0, p * 4096) if k & 1 == 0 else lds_dma(VOFF + p, S_A))
            if s == 1 and not last and k >= 12:  # A fragment addresses of K-tile t+1
                emit(f"v_add_u32 {vr(vaddr(False, g ^ 1, k - 12))}, s{S_ANEXT}, {vr(ABASE + k - 12)}")
            if s == 3 and dma:  # W piece p of K-tile t+2 -> W stage g
                emit(m0_piece(S_M0W, W_BASE + g * W_STRIDE + p * 4096) if k & 1 == 0 else lds_dma(VOFF + 8 + p, S_W))
        if s == 0 and dma:
            emit(*ptr_advance(S_A))
        if s == 1 and not last:  # rotate the A stages: K-tile t+2 reads what this K-tile's DMA wrote
            emit(f"s_mov_b32 s{S_ANEXT}, s{S_ADMA}", f"s_add_u32 s{S_ADMA}, s{S_ADMA}, {A_STRIDE}", f"s_cmp_ge_u32 s{S_ADMA}, {3 * A_STRIDE}",
                 f"s_cselect_b32 s{S_ADMA}, 0, s{S_ADMA}")
        if s == 3 and dma:
            emit(*ptr_advance(S_W))


def gen():
    L, emit = emitter(drops_opcodes(ABLATE, DROPS))
    emit("; ---- gemm_g4 K loop (generated by gen_gemm_g4.py; do not edit)")
    # prologue: K-tiles 0 and 1 whole (A0, W0, A1, W1: 32 pieces); K-tile 2's A half follows in step 0 of K-tile 0
    for t in range(2):
        for p in range(8):
            emit(m0_piece(S_M0W, t * A_STRIDE + p * 4096), "s_nop 0", lds_dma(VOFF + p, S_A))
        for p in range(8):
            emit(m0_piece(S_M0W, W_BASE + t * W_STRIDE + p * 4096), "s_nop 0", lds_dma(VOFF + 8 + p, S_W))
        emit(*ptr_advance(S_A), *ptr_advance(S_W))
    emit(f"s_mov_b32 s{S_ANEXT}, {A_STRIDE}", f"s_mov_b32 s{S_ADMA}, {2 * A_STRIDE}")
    for x in range(4):
        emit(f"v_mov_b32 {vr(ABASE + x)}, {vr(vaddr(False, 0, x))}")
    emit("s_waitcnt vmcnt(16)", "s_barrier")  # K-tile 0 landed; K-tile 1 stays in flight
    for n in range(8):
        emit(frag(0, n, 0, 0))
    # K-tile 0, s41 pairs [odd, even] (t = 1 .. nT-4), then the three last K-tiles
    emit("; K-tile 0")
    ktile(emit, 0, first=True)
    emit("L_g4_loop_%=:", f"s_cmp_eq_u32 s{S_CNT}, 0", "s_cbranch_scc1 L_g4_nopf_%=")
    ktile(emit, 1)
    ktile(emit, 0)
    emit(f"s_sub_u32 s{S_CNT}, s{S_CNT}, 1", "s_branch L_g4_loop_%=", "L_g4_nopf_%=:")
    ktile(emit, 1)                          # K-tile nT-3: the last one that stages (A and W of K-tile nT-1)
    ktile(emit, 0, dma=False)               # K-tile nT-2
    ktile(emit, 1, dma=False, last=True)
    emit("s_waitcnt vmcnt(0)", "s_nop 15", "s_nop 15")  # the epilogue reads the accumulators next
    # split K: this workgroup's partial tile goes to its slot (the stores read a[...] here, inside the statement that produced them:
    # as operands of a second statement the compiler copied all 256 accumulators out and back, with spills)
    emit(f"s_cmp_lt_u32 s{S_SK + 2}, 2", "s_cbranch_scc1 L_g4_end_%=", *gen_sk_store(f"s{S_SK}", f"s{S_SK + 1}", f"v{V_SK}"), "L_g4_end_%=:")
    return L


# ---------------------------------------------------------------------------------------------------------------------------------
# Split K (gemm_g4.hip, GemmArgs::splitk): the hand-over of the fp32 partial tiles.  Layout of one partial: [wave][64 register quads]
# [lane] x 16 bytes -- quad q of a wave = accumulator registers a[4q : 4q + 3], 1 KiB per wave and instruction.  Every access is sc1
# (device scope: written through / never served from an XCD's L2), so no L2 write-back or invalidate is needed around the arrival
# counter.  Operands: %[lo] / %[hi] = the wave's base address (SGPRs), %[voff] = lane * 16, %[ns] = number of partials (sum only).
SK_S0, SK_V0, SK_ZSTRIDE = 50, 100, 262144  # scratch SGPR pair, first of 4 x 32 scratch VGPRs, bytes between the partials of a tile


S_SK, V_SK = 44, 98  # main statement: s[44:47] = {partial slot address lo, hi, number of splits, -}, v98 = lane * 16


def gen_sk_store(lo, hi, voff):
    out = []
    for k in range(8):
        out.append(f"s_add_u32 s{SK_S0}, {lo}, {k * 8192 + 4096}")
        out.append(f"s_addc_u32 s{SK_S0 + 1}, {hi}, 0")
        for g in range(8):
            out.append(f"global_store_dwordx4 {voff}, a[{32 * k + 4 * g}:{32 * k + 4 * g + 3}], s[{SK_S0}:{SK_S0 + 1}] offset:{g * 1024 - 4096} sc1")
    out.append("s_waitcnt vmcnt(0)")  # the partial tile is in memory before the arrival is counted
    return out


def gen_sk_sum():
    """a[...] = partial 0 + partial 1 (+ partial 2 (+ partial 3)), in that order whoever runs it; the partial of the running workgroup
    (%[z]) is taken from its registers instead of memory (same bits, a third less to fetch at three splits)"""
    out = []
    for k in range(8):
        out.append(f"s_add_u32 s{SK_S0}, %[lo], {k * 8192 + 4096}")
        out.append(f"s_addc_u32 s{SK_S0 + 1}, %[hi], 0")
        for zz in range(4):
            if zz >= 2:
                out.append(f"s_cmp_lt_u32 %[ns], {zz + 1}")
                out.append(f"s_cbranch_scc1 L_sk_w{k}_%=")
            if zz:
                out.append(f"s_add_u32 s{SK_S0}, s{SK_S0}, {SK_ZSTRIDE}")
                out.append(f"s_addc_u32 s{SK_S0 + 1}, s{SK_S0 + 1}, 0")
            out.append(f"s_cmp_eq_u32 %[z], {zz}")
            out.append(f"s_cbranch_scc1 L_sk_o{k}_{zz}_%=")
            for g in range(8):
                v = SK_V0 + 32 * zz + 4 * g
                out.append(f"global_load_dwordx4 v[{v}:{v + 3}], %[voff], s[{SK_S0}:{SK_S0 + 1}] offset:{g * 1024 - 4096} sc1")
            out.append(f"s_branch L_sk_n{k}_{zz}_%=")
            out.append(f"L_sk_o{k}_{zz}_%=:")
            for i in range(32):
                out.append(f"v_accvgpr_read_b32 v{SK_V0 + 32 * zz + i}, a{32 * k + i}")
            out.append(f"L_sk_n{k}_{zz}_%=:")
        out.append(f"L_sk_w{k}_%=:")
        out.append("s_waitcnt vmcnt(0)")
        for zz in range(1, 4):
            if zz >= 2:
                out.append(f"s_cmp_lt_u32 %[ns], {zz + 1}")
                out.append(f"s_cbranch_scc1 L_sk_d{k}_%=")
            for i in range(32):
                out.append(f"v_add_f32 v{SK_V0 + i}, v{SK_V0 + i}, v{SK_V0 + 32 * zz + i}")
        out.append(f"L_sk_d{k}_%=:")
        for i in range(32):
            out.append(f"v_accvgpr_write_b32 a{32 * k + i}, v{SK_V0 + i}")
    return out


def main():
    here = out_dir(__file__)
    write_inc(os.path.join(here, "gemm_g4_body.inc"), gen())
    write_inc(os.path.join(here, "gemm_g4_sk_sum.inc"), gen_sk_sum())
    # G4_VPF (v[96:97]) and v98 / v99 in G4_CLOBBERS are what is left of the rejected L2 prefetch.  The body touches none of them, but
    # without the operand hipcc numbers the registers around the 256-accumulator statement differently, so they stay until a change that
    # re-measures the kernel anyway.
    clob = [f"v{r}" for r in range(0, 64)] + ["v98", "v99"] + [f"v{ABASE + x}" for x in range(4)] + [f"s{S_ANEXT}", f"s{S_ADMA}", f"s{S_AM0}"]
    with open(os.path.join(here, "gemm_g4_regs.h"), "w") as f:
        f.write("// generated by gen_gemm_g4.py: the physical registers the K loop of gemm_g4 owns, and its LDS size\n#pragma once\n")
        f.write(f"#define G4_LDS_BYTES {LDS_BYTES}\n")
        f.write(f"#define G4_A_STRIDE {A_STRIDE}\n#define G4_W_BASE {W_BASE}\n#define G4_W_STRIDE {W_STRIDE}  // LDS map of the operand stages: A stage g at g * A_STRIDE, W stage h at W_BASE + h * W_STRIDE\n")
        for k in range(8):
            f.write(define_regs(f"G4_ACC{k}", "a", 32 * k, 32))
        f.write(define_regs("G4_VADDR", "v", VADDR, 16) + define_regs("G4_VOFF", "v", VOFF, 16) + define_regs("G4_VPF", "v", 96, 2))
        f.write(define_regs("G4_PTR", "s", S_A, 4) + define_regs("G4_SIN", "s", S_M0W, 2))
        f.write(define_regs("G4_SK", "s", S_SK, 4) + define_regs("G4_VSK", "v", V_SK))
        f.write(define_clobbers("G4_SK_CLOBBERS", [f"v{r}" for r in range(SK_V0, SK_V0 + 128)] + [f"s{SK_S0}", f"s{SK_S0 + 1}"], ("scc", "memory")))
        f.write(define_clobbers("G4_CLOBBERS", clob + [f"s{SK_S0}", f"s{SK_S0 + 1}"]))


if __name__ == "__main__":
    main()
