// tests/emu/pred_fetch_asan.cpp -- TEST INFRASTRUCTURE: the prediction kernel's body (e264_pred.h, as pred_emu.cpp runs it) over packets that lie in heap
// blocks of EXACTLY their size, built with -fsanitize=address,undefined: a load a phase issues for a lane, a dword or a block it turns out not to need
// must still lie inside the packet -- the motion section for the motion, the macroblock's own payload for the residual -- and where that ends the packet
// the sanitizer sees any that does not.  (On the device resident packets sit in exact-size allocations too.)  A stand-alone program:
// tests/test_pred_fetch_emu.py compiles it (into its temporary directory), writes its packets to a file and runs it as a child process.
//   pred_fetch_asan FILE      FILE = { uint32 bytes, uint32 1: a new stream starts (its slots are cleared), the packet } ...
// Prints one line per packet with a sum of the destination slot; exit status 0 when every packet ran.
#include "pred_emu.cpp"

int main(int argc, char **argv)
{
	if (argc != 2) { fprintf(stderr, "usage: %s FILE\n", argv[0]); return 2; }
	FILE *f = fopen(argv[1], "rb");
	if (!f) { perror(argv[1]); return 2; }
	uint32_t head[2];
	unsigned long idx = 0;
	int bad = 0;
	uint8_t *dpb[E264_MAX_SLOTS] = {};
	size_t slot_bytes = 0;
	while (fread(head, 4, 2, f) == 2) {
		uint8_t *pkt = (uint8_t *)malloc(head[0]); // exactly the packet: what follows it is not the program's
		if (head[0] < sizeof(E264FrameHdr) || fread(pkt, 1, head[0], f) != head[0]) { fprintf(stderr, "packet %lu: short file\n", idx); return 2; }
		const E264FrameHdr *h = (const E264FrameHdr *)pkt;
		if (h->total_bytes != head[0]) { fprintf(stderr, "packet %lu: %u bytes in a block of %u\n", idx, h->total_bytes, head[0]); return 2; }
		const size_t nb = (size_t)h->plane_size_Y + h->plane_size_C;
		if (head[1] || nb != slot_bytes) { // a stream's slots: every one exists, exactly a picture large
			for (int i = 0; i < E264_MAX_SLOTS; i++) { free(dpb[i]); dpb[i] = (uint8_t *)calloc(nb, 1); }
			slot_bytes = nb;
		}
		const int r = e264emu_pred_frame2(pkt, dpb, nullptr);
		unsigned long sum = 0;
		for (size_t i = 0; i < nb; i++) sum = sum * 31 + dpb[h->dst_slot][i];
		printf("packet %lu: %d, %zu bytes, sum %lu\n", idx, r, nb, sum);
		bad |= r;
		free(pkt);
		idx++;
	}
	for (int i = 0; i < E264_MAX_SLOTS; i++) free(dpb[i]);
	fclose(f);
	return bad ? 1 : 0;
}
