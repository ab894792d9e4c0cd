// tools/sanitize/wire_fuzz.cpp -- CHECKING TOOL, host only: the wire forms of a command packet (include/edge264_compact.h, versions 5, 6 and 7) under
// AddressSanitizer + UndefinedBehaviorSanitizer, as ONE stand-alone program (nothing is loaded into an interpreter): the validation unit
// (edge264_amd/csrc/e264_check.cpp), the fold, the host expansion and e264_expand_kernel's source compiled for the host (tests/emu/pred_emu.cpp), every buffer a
// heap block of exactly the size the back end would give it, so that a read or write past an end is a report.
//
// For every version-4 packet of the capture files (tools/make_capture.py writes them; any concatenation of packets will do) and for every level of the fold (1 to 3):
//   fold -> check -> host expansion == the kernel source's expansion (grids of 256 and 1 threads) -> check of the expansion -> refold == the wire bytes,
//   then N times: damage 1..4 bytes in front of the payload; whatever e264hip_packet_check still accepts is unfolded both ways (equal bytes again) and its
//   expansion must pass the check.
// Build and run:   make -C tools/sanitize wire_fuzz && tools/sanitize/wire_fuzz capture.e264 [N=200] [seed=1]        exit status 0 = no finding
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <random>
#include <vector>
#include "../../include/edge264_hip.h"
#include "../../include/edge264_compact.h"

extern "C" int e264emu_expand(const uint8_t *wire, uint8_t *area, int nt); // tests/emu/pred_emu.cpp

static long n_fold, n_damaged, n_accepted, n_refused;

static uint8_t *heap_copy(const void *p, size_t n)
{
	uint8_t *m = (uint8_t *)malloc(n ? n : 1);
	memcpy(m, p, n);
	return m;
}

// a wire packet that has passed the check: both expansions, on exact-size blocks, byte for byte; the expansion passes the check.  The expansion (caller frees).
static uint8_t *unfold(const uint8_t *wire, size_t bytes, size_t *out_bytes, const char *what)
{
	const size_t need = e264hip_packet_expand(wire, bytes, NULL, 0);
	if (!need) { fprintf(stderr, "%s: accepted by the check, refused by the expansion: %s\n", what, e264hip_last_error()); exit(1); }
	uint8_t *x = (uint8_t *)malloc(need);
	if (e264hip_packet_expand(wire, bytes, x, need) != need) { fprintf(stderr, "%s: expansion size\n", what); exit(1); }
	if (e264hip_packet_check(x, need)) { fprintf(stderr, "%s: the expansion of an accepted packet is refused: %s\n", what, e264hip_last_error()); exit(1); }
	const E264FrameHdr *h = (const E264FrameHdr *)x;
	const size_t area_bytes = e264_expand_area_bytes(wire);
	if (area_bytes != h->payload_off - h->mbs_off) { fprintf(stderr, "%s: e264_expand_area_bytes %zu, expansion %u\n", what, area_bytes, h->payload_off - h->mbs_off); exit(1); }
	for (int nt : {256, 1}) {
		uint8_t *area = (uint8_t *)malloc(area_bytes ? area_bytes : 1);
		memset(area, 0xA5, area_bytes);
		e264emu_expand(wire, area, nt);
		if (memcmp(area, x + h->mbs_off, area_bytes)) { fprintf(stderr, "%s: kernel source and host expansion differ (grid of %d)\n", what, nt); exit(1); }
		free(area);
	}
	*out_bytes = need;
	return x;
}

int main(int argc, char **argv)
{
	if (argc < 2) { fprintf(stderr, "usage: wire_fuzz capture.e264 [mutations per packet and level] [seed]\n"); return 2; }
	const int per = argc > 2 ? atoi(argv[2]) : 200;
	std::mt19937 rng(argc > 3 ? (unsigned)atoi(argv[3]) : 1u);
	FILE *f = fopen(argv[1], "rb");
	if (!f) { perror(argv[1]); return 2; }
	std::vector<uint8_t> file;
	uint8_t chunk[65536];
	for (size_t n; (n = fread(chunk, 1, sizeof(chunk), f)) > 0;) file.insert(file.end(), chunk, chunk + n);
	fclose(f);
	for (size_t off = 0; off + sizeof(E264FrameHdr) <= file.size();) {
		const E264FrameHdr *fh = (const E264FrameHdr *)(file.data() + off);
		if (fh->magic != E264_MAGIC || fh->total_bytes < sizeof(*fh) || off + fh->total_bytes > file.size()) { fprintf(stderr, "not a command packet at offset %zu\n", off); return 2; }
		const size_t bytes = fh->total_bytes;
		uint8_t *v4 = heap_copy(fh, bytes);
		off += bytes;
		if (fh->version != E264_VERSION || e264hip_packet_check(v4, bytes)) { free(v4); continue; } // (wire packets of a capture are skipped: folded here)
		for (int level = 1; level <= 3; level++) {
			const size_t cap = e264hip_packet_fold_bound(v4, bytes, level);
			uint8_t *tmp = (uint8_t *)malloc(cap);
			const size_t wb = e264hip_packet_fold(v4, bytes, level, tmp, cap);
			if (!wb) { fprintf(stderr, "fold refused: %s\n", e264hip_last_error()); return 1; }
			uint8_t *wire = heap_copy(tmp, wb);
			n_fold++;
			if (e264hip_packet_check(wire, wb)) { fprintf(stderr, "level %d: the fold of a sound packet is refused: %s\n", level, e264hip_last_error()); return 1; }
			size_t xb;
			uint8_t *x = unfold(wire, wb, &xb, "fold");
			if (e264hip_packet_fold(x, xb, level, tmp, cap) != wb || memcmp(tmp, wire, wb)) { fprintf(stderr, "level %d: refold differs\n", level); return 1; }
			free(x);
			const uint32_t hi = ((const E264FrameHdr *)wire)->payload_off;
			for (int k = 0; k < per; k++) {
				uint8_t *bad = heap_copy(wire, wb);
				for (int j = 1 + (int)(rng() % 4); j > 0; j--) {
					const uint32_t i = rng() % hi;
					bad[i] = rng() % 10 < 7 ? (uint8_t)rng() : (uint8_t)(bad[i] ^ 1u << rng() % 8);
				}
				n_damaged++;
				if (e264hip_packet_check(bad, wb) == 0) {
					n_accepted++;
					free(unfold(bad, wb, &xb, "damaged"));
				} else
					n_refused++;
				free(bad);
			}
			free(wire);
			free(tmp);
		}
		free(v4);
	}
	printf("wire_fuzz: %ld folds (levels 1 to 3), %ld damaged packets: %ld refused, %ld accepted and unfolded on exact-size buffers; no finding\n", n_fold, n_damaged, n_refused, n_accepted);
	return n_fold ? 0 : 2;
}
