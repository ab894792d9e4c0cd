// e264_plan.cpp -- the launch rules (e264_plan.h): plain C++17, no HIP.
#include "e264_plan.h"

static const E264Form e264_forms[] = {
	{true, E264_INTRA_4, 256, E264_LC_INTRA4_BITMAP, true},
	{true, E264_INTRA_8, 512, E264_LC_INTRA8_BITMAP, true},
	{true, E264_INTRA_16, 1024, E264_LC_INTRA16_BITMAP, true},
	{false, E264_DBK_2, 128, E264_LC_DBK_2, true},
	{false, E264_DBK_4, 256, E264_LC_DBK_4, true},
	{false, E264_DBK_7, 448, E264_LC_DBK_7, true},
	{false, E264_DBK_8, 512, E264_LC_DBK_8, true},
	{false, E264_DBK2_6, 384, E264_LC_DBK2_6, true},
	{false, E264_DBK2_7, 448, E264_LC_DBK2_7, true},
	{false, E264_DBK2_8, 512, E264_LC_DBK2_8, true},
	{false, E264_DBK2_10, 640, E264_LC_DBK2_10, E264_PLAN_GS2}, // strips of four macroblocks: 12.6 KB of LDS per wave, twelve waves (three per SIMD) fit the CU
	{false, E264_DBK2_12, 768, E264_LC_DBK2_12, E264_PLAN_GS2},
};

extern "C" const E264Form *e264_form(bool intra, int value)
{
	for (const E264Form &f : e264_forms)
		if (f.intra == intra && f.value == value) return &f;
	return nullptr;
}

// (e264hip_set_option keeps the options inside the table's launchable rows; any other value runs as the launcher always ran it)
static int launchable(bool intra, int value)
{
	const E264Form *f = e264_form(intra, value);
	if (f && f->exists) return value;
	if (intra) return E264_INTRA_8;
	return f ? E264_DBK2_8 : E264_DBK_7;
}

extern "C" void e264_plan(const E264PlanIn &in, E264Plan &p)
{
	p = E264Plan();
	p.n = in.n;
	if (in.n <= 0) return;
	p.expand = in.expand;
	const E264IntraForm intra = (E264IntraForm)launchable(true, in.intra_waves);
	const E264DbkForm dbk = (E264DbkForm)launchable(false, in.waves);
	// The split-off intra pass.  Not with more than two lanes in use (unless split_intra = 2, for runs with GPU_MAX_HW_QUEUES raised): lanes and second queues then
	// share the runtime's hardware queues -- four by default -- and a lane's kernels wait behind another lane's 2.7-ms intra pass: 38.7 k against 52.0 k frames/s
	// without the split (tools/stagger_probe.py, profiles/r06_ablations.txt item 16)
	const bool split = in.recon && in.pred_work && in.has_q2 && in.n_nopred > 0 && in.n_nopred < in.n && (in.split_intra == 2 || (in.split_intra && in.max_lane < 2));
	p.n_split = split ? in.n_nopred : 0;
	// Two workgroups per picture (luma, chroma: e264_intra_planes_kernel, sixteen waves each) for the pictures whose intra pass stands alone -- while they are few: each
	// takes a whole CU (125 KB of LDS) from the prediction kernel of the others, and with more than ~320 other pictures in the submission their kernels outlast a
	// one-workgroup pass anyway (tools/stagger_probe.py: 256 pictures out of phase 72.4 -> 84.9 k frames/s; 512: 88.7 -> 86.9 k without this rule; profiles/r06_ablations.txt item 18)
	const int cu_budget = in.n_cus * 3 / 8;
	const bool planes = in.split_planes && intra == E264_INTRA_16;
	if (split) p.split = planes && 2 * in.n_nopred <= cu_budget && in.n - in.n_nopred <= 320 ? E264_INTRA_PLANES : intra;
	// ... a kernel that has the lane to itself (an all-intra batch's intra pass, every batch's deblocking) may take every CU of the lane's share (the lanes in use run
	// beside each other): 64 streams 38.2 -> 42.8 k frames/s, 128 streams 61.6 -> 69.8 k
	const int cu_alone = in.planes_alone > 0 ? in.planes_alone : in.n_cus / (in.max_lane + 1);
	const bool alone = in.split_planes && 2 * in.n <= cu_alone;
	// The parameter kernel reads nothing but the packet and is needed only by the deblocking kernel, so it can run on the second queue (unless the split-off pass has
	// it) beside the prediction kernel (side_queue 1; rounds 1 - 4: no gain, that kernel fills every CU) or beside the intra kernel (2; round 6: no gain either,
	// profiles/r06_ablations.txt item 1)
	if (in.deblock) {
		p.param = in.has_l1 ? E264_PARAM_GENERAL : E264_PARAM_SMALL;
		if (in.side_queue && in.has_q2 && !split) p.param_where = in.side_queue == 2 ? E264_PARAM_BESIDE_INTRA : E264_PARAM_BESIDE_PRED;
	}
	// An all-intra batch (every picture of an I launch) has nothing for the prediction kernel: 34 816 workgroups that load their records and leave cost 0.12 ms per
	// launch of 256 pictures; the intra kernel then scans without the bitmap those workgroups would have written
	if (in.recon && in.pred_work) {
		p.n_pred = in.n - p.n_split;
		p.pred_mode = 1 | (in.deblock ? 2 : 0) | (in.has_l1 ? 0 : 8) | (in.expand ? 16 : 0); // (the kernel ignores it: the bits it has always been handed)
	}
	if (in.recon) {
		p.intra = !in.pred_work && planes && alone ? E264_INTRA_PLANES : intra; // a FEW pictures, all without prediction work (one stream's I picture): two CUs each
		p.intra_bitmap = in.pred_work;
		p.n_intra = in.n - p.n_split;
	}
	// few pictures: two workgroups each (luma groups, chroma groups; one stream: a P picture 0.89 ms, of which the deblocking kernel is most)
	if (in.deblock) p.dbk = dbk == E264_DBK2_8 && alone ? E264_DBK_PLANES : dbk;
}

extern "C" void e264_plan_counts(const E264Plan &p, uint64_t counts[E264_LC_COUNT])
{
	auto add = [&](int slot, int n) { counts[slot] += (uint64_t)n; };
	if (p.expand) add(E264_LC_EXPAND, p.n);
	if (p.n_split) add(p.split == E264_INTRA_PLANES ? E264_LC_INTRA_PLANES_SPLIT : E264_LC_INTRA_SPLIT, p.n_split); // (any wave count: not under the kernel's own slot)
	if (p.param) add(p.param == E264_PARAM_SMALL ? E264_LC_DBKP_SMALL : E264_LC_DBKP_GENERAL, p.n);
	if (p.param_where != E264_PARAM_ON_LANE) add(p.param_where == E264_PARAM_BESIDE_PRED ? E264_LC_DBKP_SIDE1 : E264_LC_DBKP_SIDE2, p.n);
	if (p.n_pred) add(E264_LC_PRED, p.n_pred);
	if (p.intra == E264_INTRA_PLANES) add(E264_LC_INTRA_PLANES_ALONE, p.n_intra);
	else if (p.intra) add(e264_form(true, p.intra)->slot + (p.intra_bitmap ? 0 : E264_INTRA_NOBITMAP), p.n_intra);
	if (p.dbk == E264_DBK_PLANES) add(E264_LC_DBK_PLANES, p.n);
	else if (p.dbk) add(e264_form(false, p.dbk)->slot, p.n);
}
