// tools/row_form_probe.hip -- gfx950: what one lone wave pays per FP64 VALU instruction in the
// row IIR's (icw_iir_row, K1r) order-19 sample block, by operand form.
//
// The body is the block as the kernel runs it in its speculative loop (icw_row_asm.inc, orders > 17):
// a nonzero-input sample (t0 from the spare product lane, 76 VALU) and a zero-input sample (two
// row-uniform multiplies, 74 VALU), each followed by the two lane-parallel product multiplies and the
// |w| minimum; two input loads per pair, the writer lane's stores grouped behind an exec switch.
// Every term is  Y = fmac_dpp(t*1 + NC) / T = S + Y / e = T - S / NC = Y - e  with 64 active lanes and
// row_newbcast sources, in fixed registers (inline asm), so the register numbers -- hence the VGPR
// banks, reg mod 4 -- and the encodings are the probe's to choose.  A variant changes one thing:
//   (a) where the results land: fresh T and e (as shipped), e over the dead S, T rotating through
//       3 or 4 pairs (T over S with S kept as a copy costs an instruction per term and is not built:
//       the bare in-place and ping-pong dependent adds below cost the same);
//   (b) NC = Y - e as VOP2 v_fmac_f64 with the inline -1.0 against VOP3 v_add_f64 with a neg;
//       the forwarded operand in src0 against src1;
//   (c) the banks of S, T, e, NC and of the products and the 1.0;
//   (d) the non-chain instructions (products, minimum, loads) after the new w or mid-chain, and the
//       block without any memory instruction;
//   (e) the s_nop 0 the compiler puts between the term block and the product multiplies (26 of 38
//       samples in the shipped loop), and a second s_waitcnt per pair.
// Plus the bare forms the earlier probes disagree about (in-place / ping-pong dependent adds, eight
// independent accumulators, the plain four-add Kahan step).
//
// Timing: each kernel stamps s_memtime (shader cycles) and s_memrealtime (100 MHz) around its loop,
// runs >= 2 ms, and is measured after >= 2 s of back-to-back launches (and 0.25 s of itself), so the
// cycles are real cycles and the clock is reported beside them.  One workgroup of one wave, and of
// four waves (one per SIMD: K1r's placement).  The checksum is the last w: every variant of the block
// must print the same bits.
//
// Build: hipcc --offload-arch=gfx950 -O3 -o tools/row_form_probe tools/row_form_probe.hip
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <chrono>

#define CK(e) do { hipError_t e_ = (e); if (e_ != hipSuccess) { \
    fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); return 2; } } while (0)

// ---- registers (64-bit pairs; class A = banks 0/1, class B = banks 2/3) ----
#define R0   "v[0:1]"      // A
#define R1   "v[2:3]"      // B
#define R2   "v[4:5]"      // A
#define R3   "v[6:7]"      // B
#define DA   "v[8:9]"      // A
#define DB   "v[10:11]"    // B
#define NCA  "v[12:13]"    // A
#define NCB  "v[14:15]"    // B
#define SC   "v[16:17]"    // A   (an eighth accumulator of the independent adds)
#define XA0  "v[20:21]"    // A   input, two registers per nonzero sample, double-buffered
#define XB0  "v[24:25]"    // A
#define XA1  "v[28:29]"    // A
#define XB1  "v[32:33]"    // A
#define XB0b "v[26:27]"    // B
#define XB1b "v[34:35]"    // B
#define PA   "v[40:41]"    // A   products of the nonzero sample's w (rows 1, 2)
#define P2A  "v[44:45]"    // A
#define PB   "v[42:43]"    // B   products of the zero sample's w
#define P2B  "v[46:47]"    // B
#define PBa  "v[48:49]"    // A   the same in class A
#define P2Ba "v[52:53]"    // A
#define PAb  "v[50:51]"    // B   the nonzero sample's in class B
#define P2Ab "v[54:55]"    // B
#define ONEA "v[60:61]"
#define ONEB "v[62:63]"
#define PL   "v[64:65]"
#define PL2  "v[66:67]"
#define MN   "v[68:69]"
#define CV   "v[70:71]"
#define WA   "v[100:101]"  // w of the nonzero sample; WA, WB adjacent: one dwordx4 store
#define WB   "v[102:103]"
#define WAB  "v[100:103]"
#define XP   "v[124:125]"
#define OP   "v[126:127]"
#define C0   "s[56:57]"    // row-uniform c0, c1 (SGPR sources, as in the kernel)

#define CLOB "v0","v1","v2","v3","v4","v5","v6","v7","v8","v9","v10","v11","v12","v13","v14","v15","v16","v17", \
    "v18","v19","v20","v21","v22","v23","v24","v25","v26","v27","v28","v29","v30","v31","v32","v33","v34","v35", \
    "v40","v41","v42","v43","v44","v45","v46","v47","v48","v49","v50","v51","v52","v53","v54","v55","v60","v61","v62","v63", \
    "v64","v65","v66","v67","v68","v69","v70","v71","v100","v101","v102","v103","v124","v125","v126","v127", \
    "s40","s41","s44","s45","s46","s47","s48","s49","s50","s51","s52","s53","s56","s57","vcc","scc","memory"

// ---- instructions ----
#define FM(nc, p, one, l) "v_fmac_f64_dpp " nc ", " p ", " one " row_newbcast:" #l " row_mask:0xf bank_mask:0xf\n"
#define ADD(d, a, b) "v_add_f64 " d ", " a ", " b "\n"
#define SUB(d, a, b) "v_add_f64 " d ", " a ", -" b "\n"
#define MUL(d, a, b) "v_mul_f64 " d ", " a ", " b "\n"
#define NOP0 "s_nop 0\n"

// ---- one Kahan term, S -> T.  E = (D, NC, ONE) ----
// fresh T and e (the shipped form)
#define TM_F(S, T, D, NC, ONE, P, l)  FM(NC, P, ONE, l) ADD(T, S, NC) SUB(D, T, S) SUB(NC, NC, D)
// e written over S, which is dead once T exists
#define TM_A(S, T, D, NC, ONE, P, l)  FM(NC, P, ONE, l) ADD(T, S, NC) SUB(S, T, S) SUB(NC, NC, S)
// NC = NC + (-1.0) * e as VOP2
#define TM_V(S, T, D, NC, ONE, P, l)  FM(NC, P, ONE, l) ADD(T, S, NC) SUB(D, T, S) "v_fmac_f64 " NC ", -1.0, " D "\n"
#define TM_VA(S, T, D, NC, ONE, P, l) FM(NC, P, ONE, l) ADD(T, S, NC) SUB(S, T, S) "v_fmac_f64 " NC ", -1.0, " S "\n"
// the previous instruction's result in src0
#define TM_W(S, T, D, NC, ONE, P, l)  FM(NC, P, ONE, l) ADD(T, NC, S) SUB(D, T, S) "v_add_f64 " NC ", -" D ", " NC "\n"

// 16 terms (lanes 0..15) rotating through 2, 3 or 4 sum registers; products alternate between the two
// samples of the pair (PX the other sample's, PY this sample's previous).  Ends in Ra (2, 4) / Rb (3).
#define T16_2(TM, Ra, Rb, D, NC, ONE, PX, PY) \
    TM(Ra, Rb, D, NC, ONE, PX, 0) TM(Rb, Ra, D, NC, ONE, PY, 1) TM(Ra, Rb, D, NC, ONE, PX, 2) TM(Rb, Ra, D, NC, ONE, PY, 3) \
    TM(Ra, Rb, D, NC, ONE, PX, 4) TM(Rb, Ra, D, NC, ONE, PY, 5) TM(Ra, Rb, D, NC, ONE, PX, 6) TM(Rb, Ra, D, NC, ONE, PY, 7) \
    TM(Ra, Rb, D, NC, ONE, PX, 8) TM(Rb, Ra, D, NC, ONE, PY, 9) TM(Ra, Rb, D, NC, ONE, PX, 10) TM(Rb, Ra, D, NC, ONE, PY, 11) \
    TM(Ra, Rb, D, NC, ONE, PX, 12) TM(Rb, Ra, D, NC, ONE, PY, 13) TM(Ra, Rb, D, NC, ONE, PX, 14) TM(Rb, Ra, D, NC, ONE, PY, 15)
#define T16_3(TM, Ra, Rb, Rc, D, NC, ONE, PX, PY) \
    TM(Ra, Rb, D, NC, ONE, PX, 0) TM(Rb, Rc, D, NC, ONE, PY, 1) TM(Rc, Ra, D, NC, ONE, PX, 2) TM(Ra, Rb, D, NC, ONE, PY, 3) \
    TM(Rb, Rc, D, NC, ONE, PX, 4) TM(Rc, Ra, D, NC, ONE, PY, 5) TM(Ra, Rb, D, NC, ONE, PX, 6) TM(Rb, Rc, D, NC, ONE, PY, 7) \
    TM(Rc, Ra, D, NC, ONE, PX, 8) TM(Ra, Rb, D, NC, ONE, PY, 9) TM(Rb, Rc, D, NC, ONE, PX, 10) TM(Rc, Ra, D, NC, ONE, PY, 11) \
    TM(Ra, Rb, D, NC, ONE, PX, 12) TM(Rb, Rc, D, NC, ONE, PY, 13) TM(Rc, Ra, D, NC, ONE, PX, 14) TM(Ra, Rb, D, NC, ONE, PY, 15)
#define T16_4(TM, Ra, Rb, Rc, Rd, D, NC, ONE, PX, PY) \
    TM(Ra, Rb, D, NC, ONE, PX, 0) TM(Rb, Rc, D, NC, ONE, PY, 1) TM(Rc, Rd, D, NC, ONE, PX, 2) TM(Rd, Ra, D, NC, ONE, PY, 3) \
    TM(Ra, Rb, D, NC, ONE, PX, 4) TM(Rb, Rc, D, NC, ONE, PY, 5) TM(Rc, Rd, D, NC, ONE, PX, 6) TM(Rd, Ra, D, NC, ONE, PY, 7) \
    TM(Ra, Rb, D, NC, ONE, PX, 8) TM(Rb, Rc, D, NC, ONE, PY, 9) TM(Rc, Rd, D, NC, ONE, PX, 10) TM(Rd, Ra, D, NC, ONE, PY, 11) \
    TM(Ra, Rb, D, NC, ONE, PX, 12) TM(Rb, Rc, D, NC, ONE, PY, 13) TM(Rc, Rd, D, NC, ONE, PX, 14) TM(Rd, Ra, D, NC, ONE, PY, 15)
// the 16 terms split in two halves of 8, for the variants that put something mid-chain
#define T8_LO(TM, Ra, Rb, D, NC, ONE, PX, PY) \
    TM(Ra, Rb, D, NC, ONE, PX, 0) TM(Rb, Ra, D, NC, ONE, PY, 1) TM(Ra, Rb, D, NC, ONE, PX, 2) TM(Rb, Ra, D, NC, ONE, PY, 3) \
    TM(Ra, Rb, D, NC, ONE, PX, 4) TM(Rb, Ra, D, NC, ONE, PY, 5) TM(Ra, Rb, D, NC, ONE, PX, 6) TM(Rb, Ra, D, NC, ONE, PY, 7)
#define T8_HI(TM, Ra, Rb, D, NC, ONE, PX, PY) \
    TM(Ra, Rb, D, NC, ONE, PX, 8) TM(Rb, Ra, D, NC, ONE, PY, 9) TM(Ra, Rb, D, NC, ONE, PX, 10) TM(Rb, Ra, D, NC, ONE, PY, 11) \
    TM(Ra, Rb, D, NC, ONE, PX, 12) TM(Rb, Ra, D, NC, ONE, PY, 13) TM(Ra, Rb, D, NC, ONE, PX, 14) TM(Rb, Ra, D, NC, ONE, PY, 15)

// nonzero-input head (icw_row_asm.inc, I0 = 0): T = x + t0 in the input's second register, term 0's
// compensation, then term 1 from XB into Ra.  4 + 3 VALU
#define HEAD_NZ(TM, XA, XB, Ra, D, NC, ONE, P2X, PX) \
    FM(XB, P2X, ONE, 2) SUB(NC, XA, XB) FM(NC, P2X, ONE, 2) TM(XB, Ra, D, NC, ONE, PX, 0)
// zero-input head: S = c0 w[n-1], Y = c1 w[n-2], one plain Kahan step.  5 VALU
#define HEAD_Z(Ra, Rb, D, NC, W1, W2) \
    MUL(NC, C0, W2) MUL(Ra, C0, W1) ADD(Rb, Ra, NC) SUB(D, Rb, Ra) SUB(NC, NC, D)
// last term: no compensation, the sum goes to the ring register.  2 VALU
#define LAST(S, W, NC, ONE, P, l) FM(NC, P, ONE, l) ADD(W, S, NC)
// after the new w: second product row first (the next head reads it through DPP two VALU later)
#define PRODS(W, P2, P) MUL(P2, PL2, W) MUL(P, PL, W)
#define MIN(W) "v_min_f64 " MN ", " MN ", |" W "|\n"
#define LOADS(XA, XB) "global_load_dwordx2 " XA ", " XP ", off\n" "global_load_dwordx2 " XB ", " XP ", off\n"
#define WAIT(n) "s_waitcnt vmcnt(" #n ")\n"
// the writer lane's stores of four pairs, grouped as the kernel groups a block's
#define STORES "s_mov_b64 s[52:53], exec\n s_mov_b64 exec, 1\n" \
    "global_store_dwordx4 " OP ", " WAB ", off\n global_store_dwordx4 " OP ", " WAB ", off offset:16\n" \
    "global_store_dwordx4 " OP ", " WAB ", off offset:32\n global_store_dwordx4 " OP ", " WAB ", off offset:48\n" \
    "s_mov_b64 exec, s[52:53]\n"

// One pair of samples in the two-register forms: 76 + 74 VALU.
//   TM term form; Ra, Rb sum registers (Ra doubles as the input's first register's successor);
//   NOPS: what stands between the term block and the products; XA / XB: this pair's input registers
#define PAIR2(TM, XA, XB, Ra, Rb, D, NC, ONE, PAr, PBr, P2Ar, P2Br, NOPS, wn) \
    WAIT(wn) \
    HEAD_NZ(TM, XA, XB, Ra, D, NC, ONE, P2Br, PBr) T16_2(TM, Ra, Rb, D, NC, ONE, PAr, PBr) LAST(Ra, WA, NC, ONE, P2Ar, 0) \
    NOPS PRODS(WA, P2Ar, PAr) MIN(WA) LOADS(XA, XB) \
    HEAD_Z(Ra, Rb, D, NC, WA, WB) T16_2(TM, Rb, Ra, D, NC, ONE, PAr, PBr) LAST(Rb, WB, NC, ONE, P2Ar, 1) \
    NOPS PRODS(WB, P2Br, PBr) MIN(WB)
// four pairs and the stores: one loop body of 8 samples, 600 VALU.  Inputs double-buffered: the loads
// of a pair are consumed two pairs on, so the waits are vmcnt(2) behind loads and (6) behind the stores
#define BODY2(TM, XBa, XBb, Ra, Rb, D, NC, ONE, PAr, PBr, P2Ar, P2Br, NOPS) \
    PAIR2(TM, XA0, XBa, Ra, Rb, D, NC, ONE, PAr, PBr, P2Ar, P2Br, NOPS, 6) \
    PAIR2(TM, XA1, XBb, Ra, Rb, D, NC, ONE, PAr, PBr, P2Ar, P2Br, NOPS, 6) \
    PAIR2(TM, XA0, XBa, Ra, Rb, D, NC, ONE, PAr, PBr, P2Ar, P2Br, NOPS, 2) \
    PAIR2(TM, XA1, XBb, Ra, Rb, D, NC, ONE, PAr, PBr, P2Ar, P2Br, NOPS, 2) STORES

// rotation through 3 / 4 sum registers (fresh e)
#define PAIR3(XA, XB, wn) \
    WAIT(wn) \
    HEAD_NZ(TM_F, XA, XB, R0, DA, NCB, ONEA, P2B, PB) T16_3(TM_F, R0, R1, R2, DA, NCB, ONEA, PA, PB) LAST(R1, WA, NCB, ONEA, P2A, 0) \
    PRODS(WA, P2A, PA) MIN(WA) LOADS(XA, XB) \
    HEAD_Z(R0, R1, DA, NCB, WA, WB) T16_3(TM_F, R1, R2, R0, DA, NCB, ONEA, PA, PB) LAST(R2, WB, NCB, ONEA, P2A, 1) \
    PRODS(WB, P2B, PB) MIN(WB)
#define BODY3 PAIR3(XA0, XB0, 6) PAIR3(XA1, XB1, 6) PAIR3(XA0, XB0, 2) PAIR3(XA1, XB1, 2) STORES
#define PAIR4(XA, XB, wn) \
    WAIT(wn) \
    HEAD_NZ(TM_F, XA, XB, R0, DA, NCB, ONEA, P2B, PB) T16_4(TM_F, R0, R1, R2, R3, DA, NCB, ONEA, PA, PB) LAST(R0, WA, NCB, ONEA, P2A, 0) \
    PRODS(WA, P2A, PA) MIN(WA) LOADS(XA, XB) \
    HEAD_Z(R0, R1, DA, NCB, WA, WB) T16_4(TM_F, R1, R2, R3, R0, DA, NCB, ONEA, PA, PB) LAST(R1, WB, NCB, ONEA, P2A, 1) \
    PRODS(WB, P2B, PB) MIN(WB)
#define BODY4 PAIR4(XA0, XB0, 6) PAIR4(XA1, XB1, 6) PAIR4(XA0, XB0, 2) PAIR4(XA1, XB1, 2) STORES

// (d) non-chain instructions mid-chain: the nonzero sample's minimum and the loads sit between the two
// halves of the zero sample's 16 terms (the zero sample keeps its minimum behind its products: the next
// head reads P2 through DPP, which needs two VALU between the write and the read)
#define PAIR_MID(XA, XB, wn) \
    WAIT(wn) \
    HEAD_NZ(TM_F, XA, XB, R0, DA, NCB, ONEA, P2B, PB) T16_2(TM_F, R0, R2, DA, NCB, ONEA, PA, PB) LAST(R0, WA, NCB, ONEA, P2A, 0) \
    PRODS(WA, P2A, PA) \
    HEAD_Z(R0, R2, DA, NCB, WA, WB) T8_LO(TM_F, R2, R0, DA, NCB, ONEA, PA, PB) MIN(WA) LOADS(XA, XB) \
    T8_HI(TM_F, R2, R0, DA, NCB, ONEA, PA, PB) LAST(R2, WB, NCB, ONEA, P2A, 1) \
    PRODS(WB, P2B, PB) MIN(WB)
#define BODY_MID PAIR_MID(XA0, XB0, 6) PAIR_MID(XA1, XB1, 6) PAIR_MID(XA0, XB0, 2) PAIR_MID(XA1, XB1, 2) STORES
// (d) no memory instruction at all (the inputs stay what the prologue loaded)
#define PAIR_NOMEM(XA, XB) \
    HEAD_NZ(TM_F, XA, XB, R0, DA, NCB, ONEA, P2B, PB) T16_2(TM_F, R0, R2, DA, NCB, ONEA, PA, PB) LAST(R0, WA, NCB, ONEA, P2A, 0) \
    PRODS(WA, P2A, PA) MIN(WA) "v_mov_b64 " XB ", " XA "\n" \
    HEAD_Z(R0, R2, DA, NCB, WA, WB) T16_2(TM_F, R2, R0, DA, NCB, ONEA, PA, PB) LAST(R2, WB, NCB, ONEA, P2A, 1) \
    PRODS(WB, P2B, PB) MIN(WB)
#define BODY_NOMEM PAIR_NOMEM(XA0, XB0) PAIR_NOMEM(XA1, XB1) PAIR_NOMEM(XA0, XB0) PAIR_NOMEM(XA1, XB1)
// (e) a second wait per pair, before the zero-input sample
#define PAIR_W2(XA, XB, wn) \
    WAIT(wn) \
    HEAD_NZ(TM_F, XA, XB, R0, DA, NCB, ONEA, P2B, PB) T16_2(TM_F, R0, R2, DA, NCB, ONEA, PA, PB) LAST(R0, WA, NCB, ONEA, P2A, 0) \
    PRODS(WA, P2A, PA) MIN(WA) LOADS(XA, XB) WAIT(8) \
    HEAD_Z(R0, R2, DA, NCB, WA, WB) T16_2(TM_F, R2, R0, DA, NCB, ONEA, PA, PB) LAST(R2, WB, NCB, ONEA, P2A, 1) \
    PRODS(WB, P2B, PB) MIN(WB)
#define BODY_W2 PAIR_W2(XA0, XB0, 6) PAIR_W2(XA1, XB1, 6) PAIR_W2(XA0, XB0, 2) PAIR_W2(XA1, XB1, 2) STORES

// bare forms, 600 VALU per body like the block (150 x 4 instructions)
#define X4(a) a a a a
#define X5(a) a a a a a
#define X150(a) X5(X5(a a a a a a))
#define BODY_DEP_INPLACE X150(X4(ADD(R0, R0, ONEB)))
#define BODY_DEP_PINGPONG X150(ADD(R2, R0, ONEB) ADD(R0, R2, ONEB) ADD(R2, R0, ONEB) ADD(R0, R2, ONEB))
#define BODY_INDEP8 X5(X5(X5(ADD(R0, R0, ONEB) ADD(R1, R1, ONEB) ADD(R2, R2, ONEB) ADD(R3, R3, ONEB) \
                     ADD(DA, DA, ONEB) ADD(DB, DB, ONEB) ADD(NCA, NCA, ONEB) ADD(SC, SC, ONEB)))) \
                     X5(X5(X4(ADD(R0, R0, ONEB) ADD(R1, R1, ONEB))))
#define KAHAN_PLAIN(S, T) SUB(NCB, PL, DA) ADD(T, S, NCB) SUB(DA, T, S) SUB(DA, DA, NCB)
#define BODY_KAHAN_PLAIN X5(X5(X4(KAHAN_PLAIN(R0, R2) KAHAN_PLAIN(R2, R0)))) X5(X5(KAHAN_PLAIN(R0, R2) KAHAN_PLAIN(R2, R0)))
#define KAHAN_DPP(S, T) TM_F(S, T, DA, NCB, ONEA, PL, 3)
#define BODY_KAHAN_DPP X5(X5(X4(KAHAN_DPP(R0, R2) KAHAN_DPP(R2, R0)))) X5(X5(KAHAN_DPP(R0, R2) KAHAN_DPP(R2, R0)))

// prologue: constants, pointers, the inputs; the loop; the stamps.  1/64 in every coefficient lane keeps
// the recurrence bounded (19 terms of w / 64 per sample).
#define PROLOGUE \
    "v_mov_b64 " XP ", %[xp]\n v_mov_b64 " OP ", %[op]\n s_mov_b32 s40, %[it]\n" \
    "v_mov_b64 " ONEA ", 1.0\n v_mov_b64 " ONEB ", 1.0\n v_mov_b64 " CV ", 0.5\n" \
    "v_mul_f64 " CV ", " CV ", " CV "\n v_mul_f64 " CV ", " CV ", " CV "\n v_mul_f64 " CV ", " CV ", 0.5\n v_mul_f64 " CV ", " CV ", 0.5\n" \
    "v_mov_b64 " PL ", " CV "\n v_mov_b64 " PL2 ", " CV "\n v_mov_b64 " MN ", 4.0\n" \
    "s_nop 4\n v_readfirstlane_b32 s56, v70\n v_readfirstlane_b32 s57, v71\n" \
    "v_mov_b64 " R0 ", 1.0\n v_mov_b64 " R1 ", 1.0\n v_mov_b64 " R2 ", 1.0\n v_mov_b64 " R3 ", 1.0\n" \
    "v_mov_b64 " DA ", 0\n v_mov_b64 " DB ", 0\n v_mov_b64 " NCA ", 0\n v_mov_b64 " NCB ", 0\n v_mov_b64 " SC ", 1.0\n" \
    "v_mov_b64 " WA ", 1.0\n v_mov_b64 " WB ", 1.0\n" \
    "v_mov_b64 " PA ", " CV "\n v_mov_b64 " PB ", " CV "\n v_mov_b64 " P2A ", " CV "\n v_mov_b64 " P2B ", " CV "\n" \
    "v_mov_b64 " PBa ", " CV "\n v_mov_b64 " P2Ba ", " CV "\n v_mov_b64 " PAb ", " CV "\n v_mov_b64 " P2Ab ", " CV "\n" \
    "global_load_dwordx2 " XA0 ", " XP ", off\n global_load_dwordx2 " XB0 ", " XP ", off\n" \
    "global_load_dwordx2 " XB0b ", " XP ", off\n global_load_dwordx2 " XB1b ", " XP ", off\n" \
    "global_load_dwordx2 " XA1 ", " XP ", off\n global_load_dwordx2 " XB1 ", " XP ", off\n" \
    "s_waitcnt vmcnt(0)\n" \
    "s_memtime s[44:45]\n s_memrealtime s[46:47]\n s_waitcnt lgkmcnt(0)\n"
#define EPILOGUE \
    "s_memtime s[48:49]\n s_memrealtime s[50:51]\n s_waitcnt vmcnt(0) lgkmcnt(0)\n" \
    "s_mov_b64 %[t0], s[44:45]\n s_mov_b64 %[r0], s[46:47]\n s_mov_b64 %[t1], s[48:49]\n s_mov_b64 %[r1], s[50:51]\n" \
    "v_mov_b64 %[w], " WB "\n"

// x: 64 doubles (one per lane); out: 8 doubles per wave (the writer lane's 64 bytes); st: 4 stamps and
// the checksum bits per wave
#define PROBE(name, BODY) \
__global__ __launch_bounds__(256) void name(const double *x, double *out, unsigned long long *st, int iters) \
{ \
    const double *xp = x + (threadIdx.x & 63); \
    double *op = out + (threadIdx.x >> 6) * 8; \
    unsigned long long t0, t1, r0, r1; \
    double w; \
    asm volatile(PROLOGUE "1:\n" BODY "s_sub_u32 s40, s40, 1\n s_cmp_lg_u32 s40, 0\n s_cbranch_scc1 1b\n" EPILOGUE \
                 : [t0] "=&s"(t0), [r0] "=&s"(r0), [t1] "=&s"(t1), [r1] "=&s"(r1), [w] "=&v"(w) \
                 : [xp] "v"(xp), [op] "v"(op), [it] "s"(iters) : CLOB); \
    if ((threadIdx.x & 63) == 0) { \
        unsigned long long *s = st + (threadIdx.x >> 6) * 8; \
        s[0] = t0; s[1] = r0; s[2] = t1; s[3] = r1; s[4] = (unsigned long long)__double_as_longlong(w); \
    } \
}

#define N0 ""
/* as shipped: fresh T and e; S, T, e in class A and NC in class B, as the allocator places most samples */
PROBE(k_shipped_nop, BODY2(TM_F, XB0, XB1, R0, R2, DA, NCB, ONEA, PA, PB, P2A, P2B, NOP0))
PROBE(k_shipped, BODY2(TM_F, XB0, XB1, R0, R2, DA, NCB, ONEA, PA, PB, P2A, P2B, N0))
/* (a) */
PROBE(k_a_alias, BODY2(TM_A, XB0, XB1, R0, R2, DA, NCB, ONEA, PA, PB, P2A, P2B, N0))
PROBE(k_a_rot3, BODY3)
PROBE(k_a_rot4, BODY4)
/* (b) */
PROBE(k_b_vop2, BODY2(TM_V, XB0, XB1, R0, R2, DA, NCB, ONEA, PA, PB, P2A, P2B, N0))
PROBE(k_b_vop2_alias, BODY2(TM_VA, XB0, XB1, R0, R2, DA, NCB, ONEA, PA, PB, P2A, P2B, N0))
PROBE(k_b_src0, BODY2(TM_W, XB0, XB1, R0, R2, DA, NCB, ONEA, PA, PB, P2A, P2B, N0))
/* (c) everything in class A; S / T split A / B; S, T in A and e, NC in B; the products and the 1.0 in
 * NC's class */
PROBE(k_c_allA, BODY2(TM_F, XB0, XB1, R0, R2, DA, NCA, ONEA, PA, PBa, P2A, P2Ba, N0))
PROBE(k_c_stAB, BODY2(TM_F, XB0b, XB1b, R0, R1, DA, NCB, ONEA, PA, PB, P2A, P2B, N0))
PROBE(k_c_stA_eB, BODY2(TM_F, XB0, XB1, R0, R2, DB, NCB, ONEA, PA, PB, P2A, P2B, N0))
PROBE(k_c_oneB, BODY2(TM_F, XB0, XB1, R0, R2, DA, NCB, ONEB, PAb, PB, P2Ab, P2B, N0))
PROBE(k_c_alias_AB, BODY2(TM_A, XB0b, XB1b, R0, R1, DA, NCA, ONEB, PA, PB, P2A, P2B, N0))
/* (d) */
PROBE(k_d_mid, BODY_MID)
PROBE(k_d_nomem, BODY_NOMEM)
/* (e) */
PROBE(k_e_wait2, BODY_W2)
/* bare forms */
PROBE(k_dep_inplace, BODY_DEP_INPLACE)
PROBE(k_dep_pingpong, BODY_DEP_PINGPONG)
PROBE(k_indep8, BODY_INDEP8)
PROBE(k_kahan_plain, BODY_KAHAN_PLAIN)
PROBE(k_kahan_dpp, BODY_KAHAN_DPP)

typedef void (*K)(const double *, double *, unsigned long long *, int);
struct Var { const char *name; K k; int valu; int samples; };   /* per loop body */
static const Var VARS[] = {
    {"shipped+s_nop", k_shipped_nop, 600, 8}, {"shipped", k_shipped, 600, 8},
    {"a:e-over-S", k_a_alias, 600, 8}, {"a:rotate3", k_a_rot3, 600, 8}, {"a:rotate4", k_a_rot4, 600, 8},
    {"b:vop2-NC", k_b_vop2, 600, 8}, {"b:vop2-NC+e-over-S", k_b_vop2_alias, 600, 8}, {"b:fwd-in-src0", k_b_src0, 600, 8},
    {"c:all-A", k_c_allA, 600, 8}, {"c:S-A,T-B", k_c_stAB, 600, 8}, {"c:ST-A,eNC-B", k_c_stA_eB, 600, 8},
    {"c:P,one-in-NC's", k_c_oneB, 600, 8}, {"c:e-over-S,S-A,T-B", k_c_alias_AB, 600, 8},
    {"d:mid-chain", k_d_mid, 600, 8}, {"d:no-memory", k_d_nomem, 604, 8},
    {"e:second-wait", k_e_wait2, 600, 8},
    {"dep-add-inplace", k_dep_inplace, 600, 0}, {"dep-add-pingpong", k_dep_pingpong, 600, 0},
    {"indep-add-x8", k_indep8, 1200, 0}, {"kahan-4-adds", k_kahan_plain, 1000, 0}, {"kahan-dpp", k_kahan_dpp, 1000, 0},
};

static double now_s()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int main(int argc, char **argv)
{
    const int iters = argc > 1 ? atoi(argv[1]) : 2048;     /* x 8 samples x ~365 cycles = 6 M cycles: >= 2 ms */
    const double warm_s = argc > 2 ? atof(argv[2]) : 2.0;
    double *x, *out;
    unsigned long long *st, h[32];
    CK(hipMalloc(&x, 64 * 8));
    CK(hipMalloc(&out, 4 * 8 * 8));
    CK(hipMalloc(&st, 4 * 8 * 8));
    double hx[64];
    for (int i = 0; i < 64; ++i) hx[i] = 1.0;
    CK(hipMemcpy(x, hx, sizeof hx, hipMemcpyHostToDevice));
    hipDeviceProp_t p;
    CK(hipGetDeviceProperties(&p, 0));
    printf("# device %s, %d CUs, nominal clock %d kHz; %d loop bodies of 8 samples per kernel\n", p.gcnArchName,
           p.multiProcessorCount, p.clockRate, iters);
    printf("# clock = d(s_memtime) / d(s_memrealtime) x 100 MHz; cycles are s_memtime cycles of wave 0 (max over waves in [])\n");
    /* >= 2 s of back-to-back launches before the first number */
    for (double t = now_s(); now_s() - t < warm_s;) {
        for (int i = 0; i < 16; ++i) hipLaunchKernelGGL(k_shipped, dim3(1), dim3(256), 0, 0, x, out, st, iters);
        CK(hipDeviceSynchronize());
    }
    unsigned long long sum0 = 0;
    for (int waves = 1; waves <= 4; waves *= 4) {
        for (const Var &v : VARS) {
            for (double t = now_s(); now_s() - t < warm_s / 8;) {
                for (int i = 0; i < 8; ++i) hipLaunchKernelGGL(v.k, dim3(1), dim3(64 * waves), 0, 0, x, out, st, iters);
                CK(hipDeviceSynchronize());
            }
            double cyc[3], ghz[3], cmax = 0;
            for (int rep = 0; rep < 3; ++rep) {
                hipLaunchKernelGGL(v.k, dim3(1), dim3(64 * waves), 0, 0, x, out, st, iters);
                CK(hipDeviceSynchronize());
                CK(hipMemcpy(h, st, sizeof(unsigned long long) * 8 * waves, hipMemcpyDeviceToHost));
                cyc[rep] = (double)(h[2] - h[0]);
                ghz[rep] = cyc[rep] / (double)(h[3] - h[1]) * 0.1;
                for (int w = 0; w < waves; ++w) {
                    const double c = (double)(h[8 * w + 2] - h[8 * w]);
                    if (c > cmax) cmax = c;
                }
            }
            /* median of three */
            int m = (cyc[0] <= cyc[1]) ? ((cyc[1] <= cyc[2]) ? 1 : (cyc[0] <= cyc[2] ? 2 : 0))
                                       : ((cyc[0] <= cyc[2]) ? 0 : (cyc[1] <= cyc[2] ? 2 : 1));
            const double nv = (double)v.valu * iters;
            printf("%-20s waves=%d  clock %.3f GHz  %.3f cycles/VALU [%.3f]", v.name, waves, ghz[m], cyc[m] / nv, cmax / nv);
            if (v.samples) {
                printf("  %.1f cycles/sample  %.1f ns/sample  w=%016llx", cyc[m] / ((double)v.samples * iters),
                       cyc[m] / ((double)v.samples * iters) / ghz[m], h[4]);
                if (!sum0) sum0 = h[4];
                if (h[4] != sum0) printf("  CHECKSUM DIFFERS");
            }
            printf("  (%.2f ms)\n", cyc[m] / ghz[m] * 1e-6);
        }
    }
    return 0;
}
