// e264_plan.h -- which kernels a submission runs, decided on the host before anything is launched.
//
// Plain C++17 without a HIP include: the back end fills an E264PlanIn, e264_plan() applies every launch rule, the launcher
// (e264_kernels.hip e264_launch_frames) executes the E264Plan and decides nothing.  tests/test_host_logic.py builds this unit with
// the host compiler alone and compares it with the rule table of tests/test_hip_forms.py over a grid of submissions.
#ifndef E264_PLAN_H
#define E264_PLAN_H
#include <stdint.h>
#include "../../include/edge264_hip.h" // (E264_LC_*: the slots e264_plan_counts fills)

// The two wavefront kernels' forms.  A form chosen by an option carries the option's value ("intra_waves", "waves": e264_forms);
// the two-workgroups-per-picture forms are the planner's choice alone.
enum E264IntraForm { E264_INTRA_NONE = 0, E264_INTRA_PLANES = 1, E264_INTRA_4 = 4, E264_INTRA_8 = 8, E264_INTRA_16 = 16 };
enum E264DbkForm { E264_DBK_NONE = 0, E264_DBK_PLANES = 1, E264_DBK_2 = 2, E264_DBK_4 = 4, E264_DBK_7 = 7, E264_DBK_8 = 8, // e264_deblock_kernel: mixed waves
	E264_DBK2_6 = 106, E264_DBK2_7 = 107, E264_DBK2_8 = 108, E264_DBK2_10 = 110, E264_DBK2_12 = 112 }; // 100 + n: e264_deblock2_kernel, n luma / chroma waves
enum E264ParamForm { E264_PARAM_NONE, E264_PARAM_SMALL, E264_PARAM_GENERAL }; // small: no picture predicts from list 1 (e264_dbkparam2_kernel<false>)
enum E264ParamWhere { E264_PARAM_ON_LANE, E264_PARAM_BESIDE_PRED, E264_PARAM_BESIDE_INTRA }; // beside: on the lane's second queue

// One row per value of the options "waves" and "intra_waves": what e264hip_set_option accepts, what the plan names, what the launcher launches.
struct E264Form {
	bool intra;  // a row of "intra_waves" (else of "waves")
	int value;   // the option's value = the E264IntraForm / E264DbkForm
	int block;   // threads per workgroup
	int slot;    // E264_LC_* of its pictures (intra: with the bitmap; without it, E264_INTRA_NOBITMAP slots further)
	bool exists; // the kernel is part of this build (110, 112: only with strips of four macroblocks, -DE264_DBK_GS=2); set_option refuses the others
};
#define E264_INTRA_NOBITMAP (E264_LC_INTRA4_NOBITMAP - E264_LC_INTRA4_BITMAP)
#if defined(E264_DBK_GS) && E264_DBK_GS == 2
#define E264_PLAN_GS2 true
#else
#define E264_PLAN_GS2 false
#endif
extern "C" const E264Form *e264_form(bool intra, int value); // NULL: not a value of the option

struct E264PlanIn {
	// the submission
	int n, n_nopred;        // pictures; the job table's LAST n_nopred hold no inter / PCM macroblock (0: unknown or none)
	bool recon, deblock;    // what the caller asked for (E264_RUN_RECON, E264_RUN_DEBLOCK)
	bool pred_work, has_l1; // what validation learnt: some picture has inter / PCM macroblocks, some picture predicts from list 1
	bool expand;            // a wire packet is still to be unfolded on the lane
	// the device
	int split_planes, split_intra, side_queue, waves, intra_waves; // its options
	int n_cus, max_lane;    // compute units; the highest lane that has a live stream
	bool has_q2;            // the lane has a second queue
	int planes_alone;       // E264_PLANES_ALONE (A/B override of a lane's share of the compute units), 0: none
};

struct E264Plan {
	int n;                      // pictures of the submission: what the parameter and deblocking kernels (and the expansion) run over
	bool expand;                // e264_expand_kernel in front, on the lane
	// A submission that mixes pictures without prediction work (the job table's last n_split: I pictures) with others: their intra pass (one workgroup per
	// picture, 2.7 ms for a 1080p I picture) runs on the second queue from the start, beside the parameter and prediction kernels of the others, and
	// deblocking waits for both: max(intra of the I pictures, parameters + prediction + intra of the rest) instead of their sum.
	int n_split;                // 0: no split-off pass
	E264IntraForm split;        // its form: one workgroup of "intra_waves" waves, or E264_INTRA_PLANES
	E264ParamForm param;
	E264ParamWhere param_where;
	int n_pred;                 // jobs of e264_pred_kernel (the table's first), 0: not launched
	int pred_mode;              // its `mode` argument
	E264IntraForm intra;        // the lane's intra pass
	bool intra_bitmap;          // it reads the bitmap the prediction kernel wrote
	int n_intra;                // its jobs (the table's first)
	E264DbkForm dbk;
};

extern "C" void e264_plan(const E264PlanIn &in, E264Plan &plan);
// adds the plan's pictures to the slots of their forms (E264_LC_N_CUS is left alone)
extern "C" void e264_plan_counts(const E264Plan &plan, uint64_t counts[E264_LC_COUNT]);

#endif
