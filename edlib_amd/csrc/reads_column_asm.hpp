// reads_column_asm.hpp -- the column of scan_reads_kernel (reads_kernels.hip: the full-height scan of kernel A, pass 2 of the
// north-star batch) as ONE asm statement per word count.  calculateBlock (edlib.cpp:412-447) on NWD words of 32 rows as one
// long Myers word, top-down, 10 VALU ops per word; the bottom-row score moves with bit `sh` of the last word's horizontal delta.
//
// Why asm: a stream that mixes full-rate and half-rate VALU instructions issues at the sum of their rates only while its
// 8-byte instructions start at addresses that are 4 mod 8 (tools/data_ubench.hip); the compiler's column mixes 4-byte (VOP2)
// and 8-byte (VOP3) encodings, so the phase flips every few instructions: 158 SIMD cycles per 5-word column where its 35 full-
// rate + 18 half-rate instructions add up to 133 (rounds 1-5).  Here every instruction is a VOP3 encoding behind an alignment
// fence.  (The macro chains are unrolled by hand-run Python, see tools/gen_lanepair_asm.py for the pattern.)
//
// Half-rate instructions the column does without:
//   * HW, word 0: a zero comes in from row -1, so x << 1 is x + x -- two full-rate v_add_u32 where two v_alignbit_b32 stood
//     (RC_W_SH_HW: scan_reads_kernel, the banded kernel's multi-word columns and the seed verifier share it).
//   * rows built bottom-aligned (RC_SCORE_B, scan_reads_kernel<NWD, 2, true>: the dense last level of HW): the followed row is
//     bit 31 of the last word in every lane, so its delta is v_lshrrev_b32 / v_ashrrev_i32 by 31 and two v_add_u32, all full
//     rate, where the per-lane bit `sh` takes two v_bfe and a v_add3_u32.
//   * rows built bottom-aligned, two to five words (RP_*, below): Ph << 1 and Mh << 1 on register pairs, one 64-bit shift
//     where two v_alignbit_b32 stood.
// The five-word bottom-aligned column is 52 instructions: 41 full-rate, 11 half-rate (the 5 adds of the carry chain, two
// v_lshlrev_b64, two v_lshl_add_u64, the two v_alignbit_b32 of word 4), then the compare of the tracking test.  On the
// alignbit chain (RC_WORD: the other layouts, six to eight words, the banded kernel, the seed verifier) it is 54: 41 + 13
// (8 v_alignbit_b32 for words 1..4).
#pragma once

#define RC_HEAD ".p2align 3\n\ts_nop 0\n\t"
#define RC_W_A(i)        "v_and_b32_e64 %[t], %[e" #i "], %[p" #i "]\n\t"
#define RC_W_ADD0(i)     "v_add_co_u32_e64 %[s], %[cy], %[t], %[p" #i "]\n\t"
#define RC_W_ADDC(i)     "v_addc_co_u32_e64 %[s], %[cy], %[t], %[p" #i "], %[cy]\n\t"
#define RC_W_B(i, c)     "v_bitop3_b32 %[xh], %[s], %[e" #i "], %[p" #i "] bitop3:0xde\n\t" \
                         "v_bitop3_b32 %[ph" #c "], %[m" #i "], %[xh], %[p" #i "] bitop3:0xf1\n\t" \
                         "v_and_b32_e64 %[mh" #c "], %[p" #i "], %[xh]\n\t"
#define RC_W_SH(c, p)    "v_alignbit_b32 %[phs], %[ph" #c "], %[ph" #p "], 31\n\t" "v_alignbit_b32 %[mhs], %[mh" #c "], %[mh" #p "], 31\n\t"
#define RC_W_SH_HW(c)    "v_add_u32_e64 %[phs], %[ph" #c "], %[ph" #c "]\n\t" "v_add_u32_e64 %[mhs], %[mh" #c "], %[mh" #c "]\n\t"  /* row -1 of HW: hin = 0, so x << 1 = x + x (full rate) */
#define RC_W_SH_NW(c)    "v_alignbit_b32 %[phs], %[ph" #c "], -1, 31\n\t" "v_alignbit_b32 %[mhs], %[mh" #c "], 0, 31\n\t"     /* SHW / NW: hin = +1 (edlib.cpp:584,779) */
#define RC_W_C(i)        "v_or_b32_e64 %[xv], %[e" #i "], %[m" #i "]\n\t" \
                         "v_bitop3_b32 %[pn" #i "], %[mhs], %[xv], %[phs] bitop3:0xf1\n\t" \
                         "v_and_b32_e64 %[mn" #i "], %[phs], %[xv]\n\t"
#define RC_SCORE(c)      "v_bfe_u32 %[t], %[ph" #c "], %[sh], 1\n\t" "v_bfe_i32 %[s], %[mh" #c "], %[sh], 1\n\t" "v_add3_u32 %[scoreN], %[score], %[t], %[s]\n\t"
// bottom-aligned rows (scan_reads_kernel<NWD, 2, true>): the followed row is bit 31 of the last word in every lane
#define RC_SCORE_B(c)    "v_lshrrev_b32_e64 %[t], 31, %[ph" #c "]\n\t" "v_ashrrev_i32_e64 %[s], 31, %[mh" #c "]\n\t" \
                         "v_add_u32_e64 %[scoreN], %[score], %[t]\n\t" "v_add_u32_e64 %[scoreN], %[scoreN], %[s]\n\t"
#define RC_WORD0_HW      RC_W_A(0) RC_W_ADD0(0) RC_W_B(0, 0) RC_W_SH_HW(0) RC_W_C(0)
#define RC_WORD0_NW      RC_W_A(0) RC_W_ADD0(0) RC_W_B(0, 0) RC_W_SH_NW(0) RC_W_C(0)
#define RC_WORD(i, c, p) RC_W_A(i) RC_W_ADDC(i) RC_W_B(i, c) RC_W_SH(c, p) RC_W_C(i)
// (new state in registers of its own, not tied to the old: with tied operands the four bodies of the symbol dispatch each got a
// copy of the whole state in front -- 11 v_mov per 5-word column)
#define RC_OUT_W(i) [pn##i] "=&v"(Pn[i]), [mn##i] "=&v"(Mn[i])
#define RC_IN_W(i) [e##i] "v"(Eq[i]), [p##i] "v"(Pv[i]), [m##i] "v"(Mv[i])
#define RC_REST_1
#define RC_REST_2 RC_REST_1 RC_WORD(1, 1, 0)
#define RC_REST_3 RC_REST_2 RC_WORD(2, 0, 1)
#define RC_REST_4 RC_REST_3 RC_WORD(3, 1, 0)
#define RC_REST_5 RC_REST_4 RC_WORD(4, 0, 1)
#define RC_REST_6 RC_REST_5 RC_WORD(5, 1, 0)
#define RC_REST_7 RC_REST_6 RC_WORD(6, 0, 1)
#define RC_REST_8 RC_REST_7 RC_WORD(7, 1, 0)
#define RC_OUTS_1 RC_OUT_W(0)
#define RC_INS_1 RC_IN_W(0)
#define RC_OUTS_2 RC_OUTS_1, RC_OUT_W(1)
#define RC_INS_2 RC_INS_1, RC_IN_W(1)
#define RC_OUTS_3 RC_OUTS_2, RC_OUT_W(2)
#define RC_INS_3 RC_INS_2, RC_IN_W(2)
#define RC_OUTS_4 RC_OUTS_3, RC_OUT_W(3)
#define RC_INS_4 RC_INS_3, RC_IN_W(3)
#define RC_OUTS_5 RC_OUTS_4, RC_OUT_W(4)
#define RC_INS_5 RC_INS_4, RC_IN_W(4)
#define RC_OUTS_6 RC_OUTS_5, RC_OUT_W(5)
#define RC_INS_6 RC_INS_5, RC_IN_W(5)
#define RC_OUTS_7 RC_OUTS_6, RC_OUT_W(6)
#define RC_INS_7 RC_INS_6, RC_IN_W(6)
#define RC_OUTS_8 RC_OUTS_7, RC_OUT_W(7)
#define RC_INS_8 RC_INS_7, RC_IN_W(7)
#define RC_LAST_1 0
#define RC_LAST_2 1
#define RC_LAST_3 0
#define RC_LAST_4 1
#define RC_LAST_5 0
#define RC_LAST_6 1
#define RC_LAST_7 0
#define RC_LAST_8 1
#define RC_TEMPS [t] "=&v"(t_), [s] "=&v"(s_), [xh] "=&v"(xh_), [ph0] "=&v"(ph0_), [ph1] "=&v"(ph1_), [mh0] "=&v"(mh0_), [mh1] "=&v"(mh1_), [phs] "=&v"(phs_), [mhs] "=&v"(mhs_), [xv] "=&v"(xv_), [cy] "=&s"(cy_)
#define RC_SCORE_X(c) RC_SCORE(c)
#define RC_SCORE_BX(c) RC_SCORE_B(c)
#define RC_COLUMN_ASM(N, WORD0) asm(RC_HEAD WORD0 RC_REST_##N RC_SCORE_X(RC_LAST_##N) : RC_OUTS_##N, [scoreN] "=&v"(scoreN), RC_TEMPS : RC_INS_##N, [score] "v"(score), [sh] "v"(sh))
#define RC_COLUMN_ASM_B(N, WORD0) asm(RC_HEAD WORD0 RC_REST_##N RC_SCORE_BX(RC_LAST_##N) : RC_OUTS_##N, [scoreN] "=&v"(scoreN), RC_TEMPS : RC_INS_##N, [score] "v"(score))
// The pair form of the bottom-aligned column (RP_*, scan_reads_kernel<NWD, 2, true> at two to five words): Ph << 1 and Mh << 1
// on register pairs, two words per half-rate 64-bit shift.  The column is interleaved by pairs, so one pair of ph and one of mh
// is live at a time:
//   stage 1 of words 0 and 1 (t, s, xh in ONE temporary; ph0:ph1 and mh0:mh1 in the even-aligned pairs RP_PP, RP_MM);
//   cp = ph1 >> 31, cm = mh1 >> 31 (v_lshrrev_b32, full rate) into the low halves of RP_CPP / RP_CMM, whose high halves are
//   standing zeros (the kernel's `zr0`, `zr1`, inputs bound to the odd registers);
//   v_lshlrev_b64 of both pairs by 1 (HW: a zero comes in from row -1);  stage 2 of words 0 and 1 (it writes no SGPR: the
//   carry of the add chain lives on);  stage 1 of words 2, 3 and the lone word 4, the score from bit 31 of the last word;
//   v_alignbit_b32 for word 4 from ph4, ph3 BEFORE pair 2:3 is shifted in place;  v_lshl_add_u64 pair, pair, 1, {cp, 0};
//   stage 2 of words 2, 3, 4.
// Five words: 52 instructions, 41 full-rate + 11 half-rate (5 carry-chain adds, 2 v_lshlrev_b64, 2 v_alignbit_b32,
// 2 v_lshl_add_u64) against 41 + 13; two and three words trade the two v_add_u32 and two v_alignbit_b32 of words 0..1 for
// two v_lshlrev_b64, four words as five without the lone word.  A third pair would need a second carry pair (the carry out
// of pair 2:3 has to be taken before the shift that consumes the carry into it): six to eight words keep the alignbit chain.
// An asm operand cannot name the halves of a 64-bit register, so the pairs are physical registers, bound as operands
// ("{v56}") so that the compiler knows them; none of these instructions has a wait-state rule against its VALU producers or
// consumers on gfx950 (plain VALU, no SDWA / op_sel destination, no trans op, no lane select, SGPR carry read by VALU only).
#define RP_P0 "v56"
#define RP_P1 "v57"
#define RP_PP "v[56:57]"
#define RP_M0 "v58"
#define RP_M1 "v59"
#define RP_MM "v[58:59]"
#define RP_CP "v60"
#define RP_CPP "v[60:61]"
#define RP_CM "v62"
#define RP_CMM "v[62:63]"
#define RP_PL "%[phl]"
#define RP_ML "%[mhl]"
#define RP_W_A(i)          "v_and_b32_e64 %[t], %[e" #i "], %[p" #i "]\n\t"
#define RP_W_ADD0(i)       "v_add_co_u32_e64 %[t], %[cy], %[t], %[p" #i "]\n\t"
#define RP_W_ADDC(i)       "v_addc_co_u32_e64 %[t], %[cy], %[t], %[p" #i "], %[cy]\n\t"
#define RP_W_B(i, PH, MH)  "v_bitop3_b32 %[t], %[t], %[e" #i "], %[p" #i "] bitop3:0xde\n\t" \
                           "v_bitop3_b32 " PH ", %[m" #i "], %[t], %[p" #i "] bitop3:0xf1\n\t" \
                           "v_and_b32_e64 " MH ", %[p" #i "], %[t]\n\t"
#define RP_S1_0(PH, MH)    RP_W_A(0) RP_W_ADD0(0) RP_W_B(0, PH, MH)
#define RP_S1(i, PH, MH)   RP_W_A(i) RP_W_ADDC(i) RP_W_B(i, PH, MH)
#define RP_S2(i, PH, MH)   "v_or_b32_e64 %[t], %[e" #i "], %[m" #i "]\n\t" \
                           "v_bitop3_b32 %[pn" #i "], " MH ", %[t], " PH " bitop3:0xf1\n\t" \
                           "v_and_b32_e64 %[mn" #i "], " PH ", %[t]\n\t"
#define RP_CARRY           "v_lshrrev_b32_e64 " RP_CP ", 31, " RP_P1 "\n\t" "v_lshrrev_b32_e64 " RP_CM ", 31, " RP_M1 "\n\t"
#define RP_SHL             "v_lshlrev_b64 " RP_PP ", 1, " RP_PP "\n\t" "v_lshlrev_b64 " RP_MM ", 1, " RP_MM "\n\t"
#define RP_SHLADD          "v_lshl_add_u64 " RP_PP ", " RP_PP ", 1, " RP_CPP "\n\t" "v_lshl_add_u64 " RP_MM ", " RP_MM ", 1, " RP_CMM "\n\t"
#define RP_LONE            "v_alignbit_b32 " RP_PL ", " RP_PL ", " RP_P1 ", 31\n\t" "v_alignbit_b32 " RP_ML ", " RP_ML ", " RP_M1 ", 31\n\t"
#define RP_SCORE(PH, MH)   "v_lshrrev_b32_e64 %[t], 31, " PH "\n\t" "v_add_u32_e64 %[scoreN], %[score], %[t]\n\t" \
                           "v_ashrrev_i32_e64 %[t], 31, " MH "\n\t" "v_add_u32_e64 %[scoreN], %[scoreN], %[t]\n\t"
#define RP_PAIR01          RP_S1_0(RP_P0, RP_M0) RP_S1(1, RP_P1, RP_M1)
// SC: what a body does about the followed row, where the last word's Ph / Mh are still unshifted -- RP_SCORE (bit 31: the score
// moves every column), or one of the delay-row forms below (RP_SC_*).
#define RP_BODY_2(SC) RP_PAIR01 SC(RP_P1, RP_M1) RP_SHL RP_S2(0, RP_P0, RP_M0) RP_S2(1, RP_P1, RP_M1)
#define RP_BODY_3(SC) RP_PAIR01 RP_S1(2, RP_PL, RP_ML) SC(RP_PL, RP_ML) RP_LONE RP_SHL \
                  RP_S2(0, RP_P0, RP_M0) RP_S2(1, RP_P1, RP_M1) RP_S2(2, RP_PL, RP_ML)
#define RP_BODY_4(SC) RP_PAIR01 RP_CARRY RP_SHL RP_S2(0, RP_P0, RP_M0) RP_S2(1, RP_P1, RP_M1) \
                  RP_S1(2, RP_P0, RP_M0) RP_S1(3, RP_P1, RP_M1) SC(RP_P1, RP_M1) RP_SHLADD RP_S2(2, RP_P0, RP_M0) RP_S2(3, RP_P1, RP_M1)
#define RP_BODY_5(SC) RP_PAIR01 RP_CARRY RP_SHL RP_S2(0, RP_P0, RP_M0) RP_S2(1, RP_P1, RP_M1) \
                  RP_S1(2, RP_P0, RP_M0) RP_S1(3, RP_P1, RP_M1) RP_S1(4, RP_PL, RP_ML) SC(RP_PL, RP_ML) RP_LONE RP_SHLADD \
                  RP_S2(2, RP_P0, RP_M0) RP_S2(3, RP_P1, RP_M1) RP_S2(4, RP_PL, RP_ML)
#define RP_TEMPS [t] "=&v"(t_), [ph0] "=&{v56}"(ph0_), [ph1] "=&{v57}"(ph1_), [mh0] "=&{v58}"(mh0_), [mh1] "=&{v59}"(mh1_), [cy] "=&s"(cy_)
#define RP_TEMPS_LONE , [phl] "=&v"(phl_), [mhl] "=&v"(mhl_)
#define RP_TEMPS_CARRY , [cp] "=&{v60}"(cp_), [cm] "=&{v62}"(cm_)
#define RP_INS_CARRY , [z0] "{v61}"(zr0), [z1] "{v63}"(zr1)
#define RP_XT_2
#define RP_XI_2
#define RP_XT_3 RP_TEMPS_LONE
#define RP_XI_3
#define RP_XT_4 RP_TEMPS_CARRY
#define RP_XI_4 RP_INS_CARRY
#define RP_XT_5 RP_TEMPS_LONE RP_TEMPS_CARRY
#define RP_XI_5 RP_INS_CARRY
#define RP_COLUMN_ASM_B(N) asm(RC_HEAD RP_BODY_##N(RP_SCORE) : RC_OUTS_##N, [scoreN] "=&v"(scoreN), RP_TEMPS RP_XT_##N : RC_INS_##N, [score] "v"(score) RP_XI_##N)
#define RP_COLUMN_DISPATCH_B(NWD) \
    if constexpr (NWD == 2) RP_COLUMN_ASM_B(2); if constexpr (NWD == 3) RP_COLUMN_ASM_B(3); \
    if constexpr (NWD == 4) RP_COLUMN_ASM_B(4); if constexpr (NWD == 5) RP_COLUMN_ASM_B(5);
// the same column without a followed row (the band of scan_reads_banded_kernel below its full height)
#define RC_COLUMN_ASM_NS(N, WORD0) asm(RC_HEAD WORD0 RC_REST_##N : RC_OUTS_##N, RC_TEMPS : RC_INS_##N)
#define RC_COLUMN_DISPATCH_NS(NA, WORD0) \
    if constexpr (NA == 1) RC_COLUMN_ASM_NS(1, WORD0); if constexpr (NA == 2) RC_COLUMN_ASM_NS(2, WORD0); if constexpr (NA == 3) RC_COLUMN_ASM_NS(3, WORD0); \
    if constexpr (NA == 4) RC_COLUMN_ASM_NS(4, WORD0); if constexpr (NA == 5) RC_COLUMN_ASM_NS(5, WORD0); if constexpr (NA == 6) RC_COLUMN_ASM_NS(6, WORD0); \
    if constexpr (NA == 7) RC_COLUMN_ASM_NS(7, WORD0); if constexpr (NA == 8) RC_COLUMN_ASM_NS(8, WORD0);
// Delay rows (scan_reads_kernel<NWD, 2, true, R>, R = 3 or 7: rows built bottom-aligned with R all-match rows ABOVE row m-1,
// which then sits at bit 31 - R of the last word).  An all-match row copies the row above it one column late, so
// bits 31 - R .. 31 of one column's Ph / Mh are the followed row's deltas of that column and the R before it, and the score
// moves once per group of R + 1 columns, from two popcounts.  Three bodies per word count, in both forms of the column; the
// depth reaches them as two immediates, GSH = 32 - (R + 1) (28 or 24) and GBIT = 31 - R (28 or 24 as well: row m-1's own bit):
//   NONE     the first R columns of a group: no score block at all (five words: 48 instructions);
//   CAPTURE  the last: Ph >> GSH and Mh >> GSH of the last word to two outputs (two full-rate shifts), taken where the score
//            block stood -- before the last word's registers are shifted in place, which drops bit 31 -- and behind them
//            the group's update, score += popcount(nph) - popcount(nmh): two v_bcnt_u32_b32 (half rate; the first takes the
//            old score as its addend) and a subtract.  Inside the statement, so that a group's nibbles (bytes, at seven
//            rows) die with it (left to the compiler, the popcounts of a whole 16-column word sank to its end: six
//            registers, a wave at five words).  The old score stays in its register: the kernel's hit test reads both
//            (scan_reads_kernel);
//   BIT      the ragged tail of the target (up to 15 columns of the last segment): the score every column, from bit GBIT.
#define RP_SC_NONE(PH, MH)
#define RP_SC_CAPTURE(PH, MH) "v_lshrrev_b32_e64 %[nph], %[gsh], " PH "\n\t" "v_lshrrev_b32_e64 %[nmh], %[gsh], " MH "\n\t" RC_GROUP_UPDATE
#define RP_SC_BIT(PH, MH)     "v_bfe_u32 %[t], " PH ", %[gbit], 1\n\t" "v_add_u32_e64 %[scoreN], %[score], %[t]\n\t" \
                              "v_bfe_i32 %[t], " MH ", %[gbit], 1\n\t" "v_add_u32_e64 %[scoreN], %[scoreN], %[t]\n\t"
#define RP_COLUMN_ASM_D0(N, GSH, GBIT) asm(RC_HEAD RP_BODY_##N(RP_SC_NONE) : RC_OUTS_##N, RP_TEMPS RP_XT_##N : RC_INS_##N RP_XI_##N)
#define RC_GROUP_UPDATE "v_bcnt_u32_b32 %[scoreN], %[nph], %[score]\n\t" "v_bcnt_u32_b32 %[t], %[nmh], 0\n\t" \
                        "v_sub_u32_e64 %[scoreN], %[scoreN], %[t]\n\t"
#define RC_GROUP_OUTS [nph] "=&v"(nph), [nmh] "=&v"(nmh), [scoreN] "=&v"(scoreN)
#define RP_COLUMN_ASM_D1(N, GSH, GBIT) asm(RC_HEAD RP_BODY_##N(RP_SC_CAPTURE) : RC_OUTS_##N, RC_GROUP_OUTS, RP_TEMPS RP_XT_##N : RC_INS_##N, [score] "v"(score), [gsh] "n"(GSH) RP_XI_##N)
#define RP_COLUMN_ASM_D2(N, GSH, GBIT) asm(RC_HEAD RP_BODY_##N(RP_SC_BIT) : RC_OUTS_##N, [scoreN] "=&v"(scoreN), RP_TEMPS RP_XT_##N : RC_INS_##N, [score] "v"(score), [gbit] "n"(GBIT) RP_XI_##N)
#define RP_COLUMN_DISPATCH_D(F, NWD, GSH, GBIT) \
    if constexpr (NWD == 2) RP_COLUMN_ASM_D##F(2, GSH, GBIT); if constexpr (NWD == 3) RP_COLUMN_ASM_D##F(3, GSH, GBIT); \
    if constexpr (NWD == 4) RP_COLUMN_ASM_D##F(4, GSH, GBIT); if constexpr (NWD == 5) RP_COLUMN_ASM_D##F(5, GSH, GBIT);
// ... on the alignbit chain (one word, six to eight): the last word's Ph / Mh are not shifted in place there, the block stays last
#define RC_SC_CAPTURE(c)  "v_lshrrev_b32_e64 %[nph], %[gsh], %[ph" #c "]\n\t" "v_lshrrev_b32_e64 %[nmh], %[gsh], %[mh" #c "]\n\t"
#define RC_SC_BIT(c)      "v_bfe_u32 %[t], %[ph" #c "], %[gbit], 1\n\t" "v_bfe_i32 %[s], %[mh" #c "], %[gbit], 1\n\t" "v_add3_u32 %[scoreN], %[score], %[t], %[s]\n\t"
#define RC_SC_CAPTURE_X(c) RC_SC_CAPTURE(c)
#define RC_SC_BIT_X(c) RC_SC_BIT(c)
#define RC_COLUMN_ASM_D0(N, GSH, GBIT) RC_COLUMN_ASM_NS(N, RC_WORD0_HW)
#define RC_COLUMN_ASM_D1(N, GSH, GBIT) asm(RC_HEAD RC_WORD0_HW RC_REST_##N RC_SC_CAPTURE_X(RC_LAST_##N) RC_GROUP_UPDATE : RC_OUTS_##N, RC_GROUP_OUTS, RC_TEMPS : RC_INS_##N, [score] "v"(score), [gsh] "n"(GSH))
#define RC_COLUMN_ASM_D2(N, GSH, GBIT) asm(RC_HEAD RC_WORD0_HW RC_REST_##N RC_SC_BIT_X(RC_LAST_##N) : RC_OUTS_##N, [scoreN] "=&v"(scoreN), RC_TEMPS : RC_INS_##N, [score] "v"(score), [gbit] "n"(GBIT))
#define RC_COLUMN_DISPATCH_D(F, NWD, GSH, GBIT) \
    if constexpr (NWD == 1) RC_COLUMN_ASM_D##F(1, GSH, GBIT); if constexpr (NWD == 6) RC_COLUMN_ASM_D##F(6, GSH, GBIT); \
    if constexpr (NWD == 7) RC_COLUMN_ASM_D##F(7, GSH, GBIT); if constexpr (NWD == 8) RC_COLUMN_ASM_D##F(8, GSH, GBIT);
#define RC_COLUMN_DISPATCH_B(NWD, WORD0) \
    if constexpr (NWD == 1) RC_COLUMN_ASM_B(1, WORD0); if constexpr (NWD == 2) RC_COLUMN_ASM_B(2, WORD0); if constexpr (NWD == 3) RC_COLUMN_ASM_B(3, WORD0); \
    if constexpr (NWD == 4) RC_COLUMN_ASM_B(4, WORD0); if constexpr (NWD == 5) RC_COLUMN_ASM_B(5, WORD0); if constexpr (NWD == 6) RC_COLUMN_ASM_B(6, WORD0); \
    if constexpr (NWD == 7) RC_COLUMN_ASM_B(7, WORD0); if constexpr (NWD == 8) RC_COLUMN_ASM_B(8, WORD0);
#define RC_COLUMN_DISPATCH(NWD, WORD0) \
    if constexpr (NWD == 1) RC_COLUMN_ASM(1, WORD0); if constexpr (NWD == 2) RC_COLUMN_ASM(2, WORD0); if constexpr (NWD == 3) RC_COLUMN_ASM(3, WORD0); \
    if constexpr (NWD == 4) RC_COLUMN_ASM(4, WORD0); if constexpr (NWD == 5) RC_COLUMN_ASM(5, WORD0); if constexpr (NWD == 6) RC_COLUMN_ASM(6, WORD0); \
    if constexpr (NWD == 7) RC_COLUMN_ASM(7, WORD0); if constexpr (NWD == 8) RC_COLUMN_ASM(8, WORD0);
