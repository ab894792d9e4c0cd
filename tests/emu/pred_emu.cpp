// tests/emu/pred_emu.cpp -- TEST INFRASTRUCTURE.  Compiles the product's kernel source (edge264_amd/csrc/e264_pred.h, e264_dbkp.h,
// e264_dbk.h, e264_expand.h) for the host and runs the kernels' BODIES as they are, workgroup by workgroup: every thread is a
// fibre (emu_fibres.h) that meets the others at the barriers and collectives the source names -- the same arithmetic, the same
// LDS layout, the same schedule, with the VALU byte instructions restated in emu_shims.h.  tests/test_pred_emu.py, test_dbkp_emu.py
// and test_dbk_emu.py compare the results with the CPU oracle, so that a logic error is found here and not on the GPU box.
// The two places where a test looks into a body between its phases (empty on the device, e264_dev.h):
//   the parameter kernel's raw records, as they stand in LDS once they are computed; the motion area the pieces then reuse is poisoned (nothing of it may be read any more)
#define E264_EMU_DBKP_RAW(L, f, a0) do { if (g_cur == 0) { \
		if (g_raw) for (int i_ = 0; i_ < DP_MBS && (a0) + i_ < (f).wm * (f).hm; i_++) memcpy(g_raw + (size_t)((a0) + i_) * DP_RAW, (L).out[i_], DP_RAW); \
		memset((L).mo, 0xA5, sizeof((L).mo)); } \
	emu_wg_sync(); } while (0)
//   the deblocking steps that took the filter path / the copy-only path (tests check that both are exercised)
#define E264_EMU_DBK_STEP(filtered) do { if ((g_cur & 63) == 0) ((filtered) ? g_filter_steps : g_zero_steps)++; } while (0)
#include "emu_shims.h"
static uint8_t *g_raw;
static long g_zero_steps, g_filter_steps;
#include "../../edge264_amd/csrc/e264_pred.h"
#include "../../edge264_amd/csrc/e264_dbkp.h"
#include "../../edge264_amd/csrc/e264_dbk.h"
#include "../../edge264_amd/csrc/e264_expand.h"
static const E264Job *g_job; // what the workgroup being run is given: its job, and its tile / first macroblock
static int g_wg_arg;

// e264_expand_kernel over one wire packet (include/edge264_compact.h) with a grid of nt threads: area = e264_expand_area_bytes(wire)
extern "C" __attribute__((visibility("default"))) int e264emu_expand(const uint8_t *wire, uint8_t *area, int nt)
{
	E264Job job = {wire, nullptr, nullptr, area};
	for (int t = 0; t < nt; t++) expand_thread(job, (uint32_t)t, (uint32_t)nt);
	return 0;
}
static uint8_t *g_expand; // the expansion buffer the frame entry points below hand to the kernels (NULL: version-4 packets)
extern "C" __attribute__((visibility("default"))) void e264emu_set_expand(uint8_t *area) { g_expand = area; }

// dbk: NULL, or the stream's scratch (E264_SCRATCH_BYTES(macroblocks)): the kernel then also writes the intra bitmap of its tiles
extern "C" __attribute__((visibility("default"))) int e264emu_pred_frame2(const uint8_t *pkt, uint8_t *const *dpb, uint8_t *dbk)
{
	E264Job job = {pkt, dpb, dbk, g_expand};
	FrameCtx f;
	if (!open_frame(f, job))
		return -1;
	static PredLds L;
	g_job = &job;
	const int ntx = (f.wm + PT_W - 1) / PT_W, nty = (f.hm + PT_H - 1) / PT_H;
	for (g_wg_arg = 0; g_wg_arg < ntx * nty; g_wg_arg++) {
		memset(&L, 0xA5, sizeof(L)); // LDS is not zeroed on the device either
		emu_run_workgroup(PT_NT, [](int tid) { pred_kernel_body(L, *g_job, g_wg_arg, tid); });
	}
	return 0;
}
extern "C" __attribute__((visibility("default"))) int e264emu_pred_frame(const uint8_t *pkt, uint8_t *const *dpb) { return e264emu_pred_frame2(pkt, dpb, nullptr); }

// e264_dbkparam2_kernel: out = E264_DBK_BYTES per macroblock, the pieces of the deblocking lanes' layout; raw (may be NULL) = the 64-byte
// raw records (bS, alpha, beta, indexA) the pieces are made of, as they stand in LDS between the kernel's phases
template <bool HAS_L1> static int emu_dbkparam(const uint8_t *pkt, uint8_t *out, uint8_t *raw)
{
	uint8_t dummy = 0;
	uint8_t *dpb[E264_MAX_SLOTS];
	for (int i = 0; i < E264_MAX_SLOTS; i++) dpb[i] = &dummy;
	E264Job job = {pkt, dpb, out, g_expand};
	FrameCtx f;
	if (!open_frame(f, job))
		return -1;
	static DbkpLdsT<HAS_L1> L;
	g_job = &job; g_raw = raw;
	for (g_wg_arg = 0; g_wg_arg < f.wm * f.hm; g_wg_arg += DP_MBS) {
		memset(&L, 0xA5, sizeof(L));
		emu_run_workgroup(DP_NT, [](int tid) { dbkparam2_body<HAS_L1>(L, *g_job, g_wg_arg, tid); });
	}
	return 0;
}
extern "C" __attribute__((visibility("default"))) int e264emu_dbkparam_frame2(const uint8_t *pkt, uint8_t *out, uint8_t *raw) { return emu_dbkparam<true>(pkt, out, raw); }
// the kernel's small form (no room for list 1 in LDS): for pictures that do not predict from list 1 only -- the launcher's choice on the device
extern "C" __attribute__((visibility("default"))) int e264emu_dbkparam_frame2_nol1(const uint8_t *pkt, uint8_t *out, uint8_t *raw) { return emu_dbkparam<false>(pkt, out, raw); }
// the pieces alone: what e264emu_deblock_frame2 consumes
extern "C" __attribute__((visibility("default"))) int e264emu_dbkparam_frame(const uint8_t *pkt, uint8_t *out) { return e264emu_dbkparam_frame2(pkt, out, nullptr); }
// the raw records alone (64 bytes per macroblock)
extern "C" __attribute__((visibility("default"))) int e264emu_dbkparam_raw(const uint8_t *pkt, uint8_t *raw)
{
	const E264FrameHdr *h = (const E264FrameHdr *)pkt; // (vetted by open_frame in e264emu_dbkparam_frame2; a macroblock count is at most 16 bits each way)
	uint8_t *out = (uint8_t *)malloc((size_t)h->width_mbs * h->height_mbs * E264_DBK_BYTES + 1);
	const int r = e264emu_dbkparam_frame2(pkt, out, raw);
	free(out);
	return r;
}
// a raw record -> the E264_DBK_BYTES of the lanes' layout (what the kernel's piece phase does), by the slot-by-slot definition
extern "C" __attribute__((visibility("default"))) void e264emu_dbk_pieces(const uint8_t *raw, uint8_t *out)
{
	uint8_t tc0tab[4 * 52];
	for (int i = 0; i < 4 * 52; i++) tc0tab[i] = i < 52 ? 0 : c_tc0[i / 52 - 1][i % 52];
	for (int c = 0; c < 2; c++)
		for (int dir = 0; dir < 2; dir++)
			for (int sgm = 0; sgm < 4; sgm++) {
				const v2u p = dbkp_piece(raw, tc0tab, c != 0, dir, sgm);
				memcpy(out + c * 64 + sgm * 16 + dir * 8, &p, 8);
			}
	const v4u w = dbkp_mbwide(raw);
	memcpy(out + 128, &w, 16);
}
extern "C" __attribute__((visibility("default"))) int e264emu_dbk_bytes(void) { return E264_DBK_BYTES; }

// e264_deblock_kernel / e264_deblock2_kernel / e264_deblock2_planes_kernel: dbk = the parameter records (e264emu_dbkparam_frame's output);
// the picture in dpb[dst_slot] is filtered in place by the kernel's body with ONE wave (NW = 1), which takes the groups of rows in the
// order of the kernel's list: the group a group waits for (the one above it, of its own kind) is always done.
extern "C" __attribute__((visibility("default"))) void e264emu_deblock_step_counts(long *zero, long *filt, int reset)
{
	*zero = g_zero_steps; *filt = g_filter_steps;
	if (reset) g_zero_steps = g_filter_steps = 0;
}
// split: 0 = mixed waves (e264_deblock_kernel), 1 = luma waves + chroma waves (e264_deblock2_kernel),
// 2 = e264_deblock2_planes_kernel's two workgroups one after the other, chroma FIRST (the two never read each other's samples)
extern "C" __attribute__((visibility("default"))) int e264emu_deblock_frame2(const uint8_t *pkt, uint8_t *const *dpb, uint8_t *dbk, int split)
{
	E264Job job = {pkt, dpb, dbk, g_expand};
	FrameCtx f;
	if (!open_frame(f, job) || !f.dbk)
		return -1;
	static union { DkLds<1> mixed; Dk2Lds<1> two; DkPlanesLds<1> planes; } S;
	g_job = &job;
	memset(&S, 0xA5, sizeof(S));
	if (split == 0) emu_run_workgroup(64, [](int tid) { deblock_kernel_body<1>(S.mixed, *g_job, tid); });
	else if (split == 1) emu_run_workgroup(64, [](int tid) { deblock2_kernel_body<1>(S.two, *g_job, tid); });
	else {
		emu_run_workgroup(64, [](int tid) { deblock2_planes_kernel_body<1>(S.planes, *g_job, true, tid); });
		memset(&S, 0xA5, sizeof(S));
		emu_run_workgroup(64, [](int tid) { deblock2_planes_kernel_body<1>(S.planes, *g_job, false, tid); });
	}
	return 0;
}
extern "C" __attribute__((visibility("default"))) int e264emu_deblock_frame(const uint8_t *pkt, uint8_t *const *dpb, uint8_t *dbk) { return e264emu_deblock_frame2(pkt, dpb, dbk, 0); }

// the four edge slots of one lane: lines[2][20] (positions -4..15 of the lane's two lines) filtered in place; prm: a RAW 64-byte record
extern "C" __attribute__((visibility("default"))) void e264emu_dk_filter(uint8_t *lines, const uint8_t *prm, int lane, int dir)
{
	const DkRole R = dk_role<2>(lane);
	s16x2 v[20];
	for (int k = 0; k < 20; k++) v[k] = (s16x2){(short)lines[k], (short)lines[20 + k]};
	uint8_t pieces[E264_DBK_BYTES];
	e264emu_dbk_pieces(prm, pieces);
	DkRaw raw;
	memcpy(&raw.v, pieces + (R.chroma ? 64 : 0) + R.seg * 16, 8);
	memcpy(&raw.h, pieces + (R.chroma ? 64 : 0) + R.seg * 16 + 8, 8);
	memcpy(&raw.w, pieces + 128 + (R.chroma ? 8 : 0), 8);
	DkPrm P[2];
	dk_params<2>(raw, R, P);
	dk_filter<2>(v, P[dir], R);
	for (int k = 0; k < 20; k++) { // (the pack back to bytes, as dk_vpass / dk_hpass do it: p0 / q0 may arrive unclipped, E264_DBK_SATPACK)
		const uint32_t b = (E264_DBK_SATPACK && dk_is_p0q0(k)) ? v_sat_pk_u8_i16(as_u(v[k])) : v_perm(0, as_u(v[k]), 0x0c0c0200u);
		lines[k] = (uint8_t)b; lines[20 + k] = (uint8_t)(b >> 8);
	}
}
