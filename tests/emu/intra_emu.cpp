// tests/emu/intra_emu.cpp -- TEST INFRASTRUCTURE.  Compiles the product's e264_intra_kernel (edge264_amd/csrc/e264_intra.h) for the
// host AS IT IS and runs it: the 64 lanes of a wave are 64 fibres (emu_fibres.h) that run freely between the collectives and meet
// at them -- wave_sync() is a barrier, E264_BALLOT gathers one bit per lane, E264_FIRST hands out lane 0's value -- which is
// all the source assumes about a wave (lanes communicate through LDS across wave_sync only).  The picture's workgroup is ONE
// wave (the kernel's NW = 1 instantiation) taking the macroblock rows in order, so a row never waits for the row above.
// tests/test_intra_emu.py compares whole pictures with the CPU oracle: a logic error in the intra kernel is found here, on
// the host, and not on the GPU box.
#include "emu_shims.h"
static inline uint32_t v_sad_u8(uint32_t a, uint32_t b, uint32_t c)
{
	for (int i = 0; i < 4; i++) { const int d = (int)(a >> (8 * i) & 255) - (int)(b >> (8 * i) & 255); c += (uint32_t)(d < 0 ? -d : d); }
	return c;
}
static inline int relane(int lane) { return lane; }
#include "../../edge264_amd/csrc/e264_intra.h"

namespace {
IntraLds<1> g_lds;
static uint8_t *g_expand; // expansion buffer of a wire packet (include/edge264_compact.h), filled by the caller (pred_emu's e264emu_expand); NULL for version 4
extern "C" __attribute__((visibility("default"))) void e264emu_set_expand(uint8_t *area) { g_expand = area; }
const E264Job *g_job;
int g_planes = 3; // 3: e264_intra_kernel; 1 / 2: one workgroup of e264_intra_planes_kernel (luma / chroma)
void fibre_main(int lane)
{
	if (g_planes == 1) intra_kernel_body<1, 1>(g_lds, *g_job, lane);
	else if (g_planes == 2) intra_kernel_body<1, 2>(g_lds, *g_job, lane);
	else intra_kernel_body<1>(g_lds, *g_job, lane);
}
} // namespace

// e264_intra_kernel<1> on one picture: every intra macroblock of the packet is reconstructed into dpb[dst_slot]
// scratch: NULL (every chunk of every row is scanned), or the stream's scratch with the intra bitmap e264_pred_kernel has left there
// (tests/emu/pred_emu.cpp e264emu_pred_frame2 on the same packet): rows and chunks without a bit are left alone
extern "C" __attribute__((visibility("default"))) int e264emu_intra_frame2(const uint8_t *pkt, uint8_t *const *dpb, uint8_t *scratch)
{
	const E264Job job = {pkt, dpb, scratch, g_expand};
	FrameCtx f;
	if (!open_frame(f, job))
		return -1;
	g_job = &job;
	memset(&g_lds, 0xA5, sizeof(g_lds)); // LDS is not zeroed on the device either
	emu_run_workgroup(64, fibre_main);
	return 0;
}
extern "C" __attribute__((visibility("default"))) int e264emu_intra_frame(const uint8_t *pkt, uint8_t *const *dpb) { return e264emu_intra_frame2(pkt, dpb, nullptr); }

// e264_intra_planes_kernel on one picture: its two workgroups one after the other -- chroma FIRST, so that a chroma sample that needed a luma one (none may) would find it missing
extern "C" __attribute__((visibility("default"))) int e264emu_intra_frame_planes(const uint8_t *pkt, uint8_t *const *dpb)
{
	g_planes = 2;
	int r = e264emu_intra_frame2(pkt, dpb, nullptr);
	g_planes = 1;
	if (!r) r = e264emu_intra_frame2(pkt, dpb, nullptr);
	g_planes = 3;
	return r;
}
