// e264_kernels.hip -- gfx950 (MI355X) macroblock reconstruction kernels.
//
// Consumes the command packet of include/edge264_cmd.h and writes the planar YUV DPB.
// Device restatement of the reference's sample path (file:line in /root/reference/src):
//   residual   edge264_residual.c:108-538   (dequant + 4x4 / 8x8 integer IDCT, DC transforms)
//   intra      edge264_intra.c:291-765      (14 + 32 + 7 + 7 internal modes)
//   inter      edge264_inter.c:416-1251     (6-tap luma, bilinear chroma, 5 weighting schemes)
//   deblock    edge264_deblock.c:927-1123   (bS / alpha / beta / tC0) and :284-895 (filters)
//
// Execution model, four launches per batch of frames (one frame of each of n streams):
//   e264_dbkparam2_kernel (e264_dbkp.h)  one workgroup per 64 macroblocks: deblocking parameters (bS, alpha, beta, indexA)
//                        of EVERY macroblock from the command packet alone (nothing in the frame is read).
//   e264_pred_kernel (e264_pred.h)       one workgroup per tile of 16 x 4 macroblocks, one lane per 8x8 block: inter
//                        prediction + residual (+ PCM), which depend on nothing inside the frame.
//   e264_intra_kernel (e264_intra.h)     ONE WORKGROUP PER FRAME, ONE WAVE PER MACROBLOCK ROW: intra MBs only, row y
//                        may reconstruct macroblock x once row y-1 has finished macroblock x+1.
//   e264_deblock2_kernel (e264_dbk.h)    one workgroup per frame, eight waves that take groups of 8 luma rows and of 16 chroma rows
//                        from one list, two lines per lane: the raster dependency order of H.264 in-loop deblocking
//                        (SURVEY.md 8a a16).  e264_deblock_kernel (option "waves" below 100) is the earlier form: five rows per wave, luma and chroma.
// Which form of each a submission gets (wave counts, two workgroups per picture, the second queue) is decided on the host: e264_plan.h.
// Progress counters live in LDS, so the hand-off between rows never leaves the CU: no
// agent-scope fences, no cross-XCD traffic, no placement assumption.  Chip-level parallelism
// comes from many independent streams (one frame of each per launch), the north-star workload
// (>=1000 concurrent streams).  Integer / byte work throughout, no MFMA.
//
// Pipeline rule (learnt with the phase profiler, -DE264_PHASE_TIMING / tools/visits/gpu_phase.sh): a stage that ISSUES loads for
// a later stage must not read, clear or copy any register that may still have a load in flight -- each of those is an
// s_waitcnt vmcnt(0), i.e. a wait for the loads it has just issued.  Hence: prefetch helpers contain loads only, nothing
// is zero-initialised in front of a conditional load, one code path fills the pipeline registers, and the place where
// the prefetches are consumed says so with an explicit vmcnt(0).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/edge264_cmd.h"
#include "e264_kernels.h"
#include "e264_dev.h"
#include "e264_pred.h"
#include "e264_dbkp.h"
#include "e264_dbk.h"
#include "e264_intra.h"
#include "e264_expand.h"

// XCD-aware workgroup order.  The dispatcher places linear workgroup b on XCD b % 8, each with a private
// 4 MiB L2; in launch order the strips that share reference rows (vertical neighbours of one frame,
// 15 strips = 4 workgroups apart) land on different XCDs and every one of them fetches the shared
// halo lines from HBM again.  This bijective remap gives each XCD a contiguous range of (frame, strip)
// pairs, so a frame is walked by ONE XCD and the halo rows are L2 hits.  Pure speed choice.
static __device__ __forceinline__ void xcd_tile(int &bx, int &by)
{
	const unsigned gx = gridDim.x, nwg = gx * gridDim.y;
	const unsigned lin = blockIdx.y * gx + blockIdx.x;
	const unsigned q = nwg >> 3, r = nwg & 7, xcd = lin & 7;
	const unsigned v = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (lin >> 3);
	by = (int)(v / gx);
	bx = (int)(v - (unsigned)by * gx);
}

// Inter prediction + residual of every inter / PCM macroblock: one workgroup per tile of 16 x PT_H macroblocks, one thread
// per 8x8 block; the body is in e264_pred.h (and run on the host by tests/emu).
#ifndef E264_PRED_WAVES_PER_EU
#define E264_PRED_WAVES_PER_EU 4 // 128 VGPRs: 16 waves per CU (four 256-thread workgroups), so that one tile's barriers and first loads hide behind the others' arithmetic
#endif
__attribute__((amdgpu_waves_per_eu(E264_PRED_WAVES_PER_EU, E264_PRED_WAVES_PER_EU))) __global__ __launch_bounds__(PT_NT) void e264_pred_kernel(const E264Job *jobs, int mode)
{
	__shared__ PredLds L;
	int bx, by;
	xcd_tile(bx, by);
	pred_kernel_body(L, jobs[by], bx, (int)threadIdx.x);
}

// Deblocking parameters of every macroblock, 64 consecutive macroblocks per workgroup: records in through LDS with
// contiguous 16-byte loads, parameters out as contiguous 16-byte stores (the body is in e264_dbkp.h and runs on the host in tests/emu).
// Two forms of one kernel (e264_dbkp.h): <false> for batches the launcher knows to be without list-1 motion (18.6 KB of LDS, 52 VGPRs as the compiler likes them: eight
// workgroups per CU), <true> the general one -- 19.9 KB, and held to 64 VGPRs (two of them spill) so that the register file, too, takes eight workgroups
template <bool HAS_L1> __global__ void e264_dbkparam2_kernel(const E264Job *jobs);
template <> __global__ __launch_bounds__(DP_NT) void e264_dbkparam2_kernel<false>(const E264Job *jobs)
{
	__shared__ DbkpLdsT<false> L;
	int bx, by;
	xcd_tile(bx, by);
	dbkparam2_body<false>(L, jobs[by], bx * DP_MBS, (int)threadIdx.x);
}
template <> __attribute__((amdgpu_waves_per_eu(8, 8))) __global__ __launch_bounds__(DP_NT) void e264_dbkparam2_kernel<true>(const E264Job *jobs)
{
	__shared__ DbkpLdsT<true> L;
	int bx, by;
	xcd_tile(bx, by);
	dbkparam2_body<true>(L, jobs[by], bx * DP_MBS, (int)threadIdx.x);
}

template <int NW>
__global__ __launch_bounds__(NW * 64) void e264_intra_kernel(const E264Job *jobs, int use_bitmap)
{
	__shared__ IntraLds<NW> S;
	intra_kernel_body<NW>(S, jobs[blockIdx.x], (int)threadIdx.x, use_bitmap != 0);
}
// The same pass with a picture's LUMA and CHROMA on two workgroups (blockIdx.y): intra prediction and residual of the two never meet (a chroma block predicts from
// chroma samples only), so an I picture whose intra pass stands alone on the critical path -- a submission that mixes it with P / B pictures (E264Plan.n_split), one
// stream by itself -- gets two CUs instead of one.  Sixteen waves each; no bitmap (pictures without prediction work).
__global__ __launch_bounds__(1024) void e264_intra_planes_kernel(const E264Job *jobs)
{
	__shared__ IntraLds<16> S;
	if (blockIdx.y == 0) intra_kernel_body<16, 1>(S, jobs[blockIdx.x], (int)threadIdx.x, false);
	else intra_kernel_body<16, 2>(S, jobs[blockIdx.x], (int)threadIdx.x, false);
}

// In-loop deblocking, one workgroup per picture: the bodies are in e264_dbk.h (and run on the host by tests/emu).
template <int NW> __global__ __launch_bounds__(NW * 64) void e264_deblock_kernel(const E264Job *jobs)
{
	__shared__ DkLds<NW> S;
	deblock_kernel_body<NW>(S, jobs[blockIdx.x], (int)threadIdx.x);
}
template <int NW> __global__ __launch_bounds__(NW * 64) void e264_deblock2_kernel(const E264Job *jobs)
{
	__shared__ Dk2Lds<NW> S;
	deblock2_kernel_body<NW>(S, jobs[blockIdx.x], (int)threadIdx.x);
}
template <int NW> __global__ __launch_bounds__(NW * 64) void e264_deblock2_planes_kernel(const E264Job *jobs) // blockIdx.y: luma groups, chroma groups
{
	__shared__ DkPlanesLds<NW> S;
	deblock2_planes_kernel_body<NW>(S, jobs[blockIdx.x], blockIdx.y != 0, (int)threadIdx.x);
}

// Build-time switches this code object was compiled with, as a space-separated list ("" = the product build).  The timing
// ablations (E264_ABL_*, E264_PHASE_*) produce WRONG SAMPLES on purpose: a library that reports one is refused by every loader
// (e264hip_device_open, edge264_amd/backend.py, the front end) unless E264_ALLOW_ABLATION=1 is set -- the A/B tooling sets it.
extern "C" const char *e264_kernel_build_flags(void)
{
	return ""
#if E264_DBK_GS == 2 // (not an ablation: a bit-exact variant; named so that the back end knows which wave counts exist)
		" E264_DBK_GS=2"
#endif
#ifdef E264_ABL_NOBH
		" E264_ABL_NOBH"
#endif
#ifdef E264_ABL_NOEDGE
		" E264_ABL_NOEDGE"
#endif
#ifdef E264_ABL_NOLOAD
		" E264_ABL_NOLOAD"
#endif
#ifdef E264_ABL_NOLUMA
		" E264_ABL_NOLUMA"
#endif
#ifdef E264_ABL_DBKP_NOMOT
		" E264_ABL_DBKP_NOMOT"
#endif
#ifdef E264_ABL_DBK_NOFILTER
		" E264_ABL_DBK_NOFILTER"
#endif
#ifdef E264_ABL_DBK_NOLOAD
		" E264_ABL_DBK_NOLOAD"
#endif
#ifdef E264_ABL_DBK_NOSTORE
		" E264_ABL_DBK_NOSTORE"
#endif
#ifdef E264_ABL_INTRA_NOWAIT
		" E264_ABL_INTRA_NOWAIT"
#endif
#ifdef E264_ABL_INTRA_STOP
		" E264_ABL_INTRA_STOP"
#endif
#ifdef E264_ABL_DBKP_STORE1
		" E264_ABL_DBKP_STORE1"
#endif
#ifdef E264_ABL_DBKP_NOPIECES
		" E264_ABL_DBKP_NOPIECES"
#endif

#ifdef E264_ABL_INTRA_NOFENCE
		" E264_ABL_INTRA_NOFENCE"
#endif
#ifdef E264_ABL_DBK_NOWAIT
		" E264_ABL_DBK_NOWAIT"
#endif
#ifdef E264_PHASE_TIMING
		" E264_PHASE_TIMING"
#endif
#ifdef E264_DBK_TIMELINE
		" E264_DBK_TIMELINE"
#endif
#ifdef E264_PHASE_INTRA
		" E264_PHASE_INTRA"
#endif
#ifdef E264_PRED_HPAIR
		" E264_PRED_HPAIR"
#endif
#ifdef E264_PRED_CHROMA_LAST
		" E264_PRED_CHROMA_LAST"
#endif
#ifdef E264_PRED_CLASS_PACKED
		" E264_PRED_CLASS_PACKED"
#endif
		;
}

// ---------------------------------------------------------------------------------
// Kernel 0 (only for batches with wire packets): version 5, 6 or 7 -> the record array and motion section of version 4 (e264_expand.h)
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(XP_NT) void e264_expand_kernel(const E264Job *jobs)
{
	expand_thread(jobs[blockIdx.y], blockIdx.x * XP_NT + threadIdx.x, gridDim.x * XP_NT);
}

extern "C" int e264_pred_tiles(int width_mbs, int height_mbs)
{
	return ((width_mbs + PT_W - 1) / PT_W) * ((height_mbs + PT_H - 1) / PT_H);
}

extern "C" hipError_t e264_launch_expand(const E264Job *jobs, int n_jobs, int max_mbs, hipStream_t stream)
{
	if (n_jobs > 0)
		hipLaunchKernelGGL(e264_expand_kernel, dim3((max_mbs + XP_NT - 1) / XP_NT, n_jobs), dim3(XP_NT), 0, stream, jobs);
	return hipGetLastError();
}

// ---------------------------------------------------------------------------------
// The launcher: executes an E264Plan (e264_plan.h), decides nothing
// ---------------------------------------------------------------------------------
static_assert(E264_PLAN_GS2 == (E264_DBK_GS == 2), "e264_plan.h and e264_dbk.h disagree about E264_DBK_GS");

// the kernel of a row of e264_forms
typedef void (*E264IntraKernel)(const E264Job *, int);
static E264IntraKernel intra_kernel(E264IntraForm form)
{
	switch (form) {
	case E264_INTRA_4: return e264_intra_kernel<4>;
	case E264_INTRA_16: return e264_intra_kernel<16>;
	default: return e264_intra_kernel<8>;
	}
}
typedef void (*E264DbkKernel)(const E264Job *);
static E264DbkKernel dbk_kernel(E264DbkForm form)
{
	switch (form) {
	case E264_DBK_PLANES: return e264_deblock2_planes_kernel<8>;
#if E264_DBK_GS == 2
	case E264_DBK2_12: return e264_deblock2_kernel<12>;
	case E264_DBK2_10: return e264_deblock2_kernel<10>;
#endif
	case E264_DBK2_8: return e264_deblock2_kernel<8>;
	case E264_DBK2_7: return e264_deblock2_kernel<7>;
	case E264_DBK2_6: return e264_deblock2_kernel<6>;
	case E264_DBK_2: return e264_deblock_kernel<2>;
	case E264_DBK_4: return e264_deblock_kernel<4>;
	case E264_DBK_8: return e264_deblock_kernel<8>;
	default: return e264_deblock_kernel<7>;
	}
}

// the intra pass of n jobs on queue q
static void launch_intra(E264IntraForm form, const E264Job *jobs, int n, hipStream_t q, int use_bitmap)
{
	if (form == E264_INTRA_PLANES) hipLaunchKernelGGL(e264_intra_planes_kernel, dim3(n, 2), dim3(1024), 0, q, jobs);
	else hipLaunchKernelGGL(intra_kernel(form), dim3(n), dim3(e264_form(true, form)->block), 0, q, jobs, use_bitmap);
}
// the parameter kernel on queue q
static void launch_param(E264ParamForm form, const E264Job *jobs, int n, int max_mbs, hipStream_t q)
{
	const dim3 grid((max_mbs + DP_MBS - 1) / DP_MBS, n);
	if (form == E264_PARAM_SMALL) hipLaunchKernelGGL(e264_dbkparam2_kernel<false>, grid, dim3(DP_NT), 0, q, jobs);
	else hipLaunchKernelGGL(e264_dbkparam2_kernel<true>, grid, dim3(DP_NT), 0, q, jobs);
}
// One kernel on the second queue from this point of the lane on; the lane waits for fork.joined where it needs the result
template <class Launch>
static void launch_beside(const E264Fork &fork, hipStream_t stream, bool marks, Launch launch)
{
	hipEventRecord(fork.forked, stream);
	hipStreamWaitEvent(fork.aux, fork.forked, 0);
	if (marks) hipEventRecord(fork.amarks[0], fork.aux);
	launch(fork.aux);
	if (marks) hipEventRecord(fork.amarks[1], fork.aux);
	hipEventRecord(fork.joined, fork.aux);
}

extern "C" hipError_t e264_launch_frames(const E264Job *jobs, int n_jobs, int max_mbs, int max_tiles, const E264Plan &plan, hipStream_t stream, hipEvent_t *marks,
	const E264Fork &fork)
{
	if (n_jobs <= 0)
		return hipSuccess;
	// wire packets first (before the marks: they bracket the four kernels; the whole-run clocks contain this one)
	if (plan.expand) {
		const hipError_t e = e264_launch_expand(jobs, n_jobs, max_mbs, stream);
		if (e != hipSuccess)
			return e;
	}
	// marks (optional): 5 events recorded before / between / after the four launches
	if (marks) hipEventRecord(marks[0], stream);
	// the split-off pictures (the table's last n_split) start NOW on the second queue; up to deblocking the lane sees the other jobs only
	if (plan.n_split)
		launch_beside(fork, stream, marks, [&](hipStream_t q) { launch_intra(plan.split, jobs + n_jobs - plan.n_split, plan.n_split, q, 0); });
	auto param_beside = [&]() { launch_beside(fork, stream, marks, [&](hipStream_t q) { launch_param(plan.param, jobs, n_jobs, max_mbs, q); }); };
	if (plan.param_where == E264_PARAM_BESIDE_PRED) param_beside();
	else if (plan.param && plan.param_where == E264_PARAM_ON_LANE) launch_param(plan.param, jobs, n_jobs, max_mbs, stream);
	if (marks) hipEventRecord(marks[1], stream);
	if (plan.n_pred) hipLaunchKernelGGL(e264_pred_kernel, dim3(max_tiles, plan.n_pred), dim3(PT_NT), 0, stream, jobs, plan.pred_mode);
	if (marks) hipEventRecord(marks[2], stream);
	if (plan.param_where == E264_PARAM_BESIDE_INTRA) param_beside();
	if (plan.intra) launch_intra(plan.intra, jobs, plan.n_intra, stream, plan.intra_bitmap);
	if (plan.n_split || plan.param_where != E264_PARAM_ON_LANE) hipStreamWaitEvent(stream, fork.joined, 0); // (before the mark: with the parameter kernel beside it, "intra" is the phase both share)
	if (marks) hipEventRecord(marks[3], stream);
	const bool planes = plan.dbk == E264_DBK_PLANES; // two workgroups of eight waves per picture: luma groups, chroma groups
	if (plan.dbk) hipLaunchKernelGGL(dbk_kernel(plan.dbk), dim3(n_jobs, planes ? 2 : 1), dim3(planes ? 512 : e264_form(false, plan.dbk)->block), 0, stream, jobs);
	if (marks) hipEventRecord(marks[4], stream);
	return hipGetLastError();
}

#if defined(E264_PHASE_TIMING) || defined(E264_DBK_TIMELINE)
extern "C" __attribute__((visibility("default"))) int e264_debug_phase_cycles(unsigned long long *out32, int reset)
{
	hipDeviceSynchronize();
	if (out32 && hipMemcpyFromSymbol(out32, HIP_SYMBOL(g_phase), sizeof(g_phase)) != hipSuccess) return -1;
	if (out32 && hipMemcpyFromSymbol(out32 + 32, HIP_SYMBOL(g_timeline), sizeof(g_timeline)) != hipSuccess) return -1; // the caller has room for 32 + 128
	if (reset) { unsigned long long z[32] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_phase), z, sizeof(z)) != hipSuccess) return -1; }
	return 0;
}
#endif
