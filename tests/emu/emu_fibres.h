// tests/emu/emu_fibres.h -- TEST INFRASTRUCTURE: the workgroup the kernels' bodies run in on the host.  Every thread is a fibre
// (ucontext) that runs freely between the collectives and meets the others at them: emu_wg_sync() is the workgroup's barrier,
// wave_sync() the barrier of a group of 64, emu_ballot / emu_first / emu_wg_or gather one bit per thread or hand out lane 0's
// value -- which is all the source assumes about a wave and a workgroup (threads communicate through LDS across barriers only).
// Shared by pred_emu.cpp and intra_emu.cpp through emu_shims.h.
#ifndef E264_EMU_FIBRES_H
#define E264_EMU_FIBRES_H
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <ucontext.h>

namespace {
enum { EMU_MAX_THREADS = 256, EMU_STACK = 512 * 1024 };
struct EmuBarrier { int alive, arrived; unsigned gen; };
ucontext_t g_main, g_ctx[EMU_MAX_THREADS];
char *g_stack[EMU_MAX_THREADS];
bool g_done[EMU_MAX_THREADS];
int g_cur, g_threads;
void (*g_body)(int tid);
struct { // the barriers, and the collectives' rotating slots: a thread may be one call ahead of the others
	EmuBarrier wg, wave[EMU_MAX_THREADS / 64];
	unsigned first_cnt[EMU_MAX_THREADS], bal_cnt[EMU_MAX_THREADS], or_cnt[EMU_MAX_THREADS];
	uint32_t first_val[EMU_MAX_THREADS / 64][3];
	unsigned long long bal[EMU_MAX_THREADS / 64][3];
	bool wg_or[3];
} g_wg;

void switch_to_next()
{ // round-robin: the next fibre that has not finished (this one, if it is the only one left, just goes on)
	const int from = g_cur;
	for (int k = 1; k <= g_threads; k++) {
		const int n = (from + k) % g_threads;
		if (g_done[n]) continue;
		if (n == from) return;
		g_cur = n;
		swapcontext(&g_ctx[from], &g_ctx[n]);
		return;
	}
}
void emu_barrier(EmuBarrier &b)
{
	const unsigned gen = b.gen;
	if (++b.arrived == b.alive) { b.arrived = 0; b.gen++; return; } // the last one to arrive releases everybody
	while (b.gen == gen) switch_to_next();
}
void emu_fibre_main(int tid)
{
	g_body(tid);
	g_done[tid] = true; // a thread that has returned no longer counts (the threads of a wave, or of the workgroup, leave together)
	EmuBarrier *const mine[2] = {&g_wg.wave[tid >> 6], &g_wg.wg};
	for (EmuBarrier *b : mine)
		if (--b->alive > 0 && b->arrived == b->alive) { b->arrived = 0; b->gen++; }
	for (int k = 1; k < g_threads; k++) {
		const int n = (tid + k) % g_threads;
		if (!g_done[n]) { g_cur = n; setcontext(&g_ctx[n]); }
	}
	setcontext(&g_main);
}
// one workgroup of n threads (whole waves), each running body(tid), to its end
void emu_run_workgroup(int n, void (*body)(int tid))
{
	if (n <= 0 || n > EMU_MAX_THREADS || n % 64) { fprintf(stderr, "emu: a workgroup of %d threads\n", n); abort(); }
	g_body = body; g_threads = n;
	memset(&g_wg, 0, sizeof(g_wg));
	g_wg.wg.alive = n;
	for (int tid = 0; tid < n; tid++) {
		g_wg.wave[tid >> 6].alive = 64;
		if (!g_stack[tid]) g_stack[tid] = (char *)malloc(EMU_STACK);
		g_done[tid] = false;
		getcontext(&g_ctx[tid]);
		g_ctx[tid].uc_stack.ss_sp = g_stack[tid];
		g_ctx[tid].uc_stack.ss_size = EMU_STACK;
		g_ctx[tid].uc_link = &g_main;
		makecontext(&g_ctx[tid], (void (*)())emu_fibre_main, 1, tid);
	}
	g_cur = 0;
	swapcontext(&g_main, &g_ctx[0]);
}
} // namespace

static inline void wave_sync() { emu_barrier(g_wg.wave[g_cur >> 6]); }
static inline void emu_wg_sync() { emu_barrier(g_wg.wg); }
static inline uint32_t emu_first(uint32_t v)
{ // v_readfirstlane: every lane is active wherever the kernels use it, so "first" is lane 0
	const unsigned n = g_wg.first_cnt[g_cur]++ % 3;
	if ((g_cur & 63) == 0) g_wg.first_val[g_cur >> 6][n] = v;
	wave_sync();
	return g_wg.first_val[g_cur >> 6][n];
}
static inline unsigned long long emu_ballot(bool p)
{
	const unsigned n = g_wg.bal_cnt[g_cur]++ % 3;
	if ((g_cur & 63) == 0) g_wg.bal[g_cur >> 6][(n + 1) % 3] = 0; // the slot of the NEXT ballot: nobody is there yet, everybody has left its previous use
	if (p) g_wg.bal[g_cur >> 6][n] |= 1ull << (g_cur & 63);
	wave_sync();
	return g_wg.bal[g_cur >> 6][n];
}
static inline bool emu_wg_or(bool p)
{ // __syncthreads_or: the barrier, and whether any thread of the workgroup came with a true p
	const unsigned n = g_wg.or_cnt[g_cur]++ % 3;
	if (g_cur == 0) g_wg.wg_or[(n + 1) % 3] = false;
	if (p) g_wg.wg_or[n] = true;
	emu_wg_sync();
	return g_wg.wg_or[n];
}
#endif
