// tests/emu/motion_fetch_asan.cpp -- TEST INFRASTRUCTURE: the parameter kernel's body (e264_dbkp.h, as pred_emu.cpp runs it) over packets that
// lie in heap blocks of EXACTLY their size, built with -fsanitize=address,undefined: a load the kernel issues for a lane or dword it turns out
// not to need must still lie inside the packet's motion section, and where that section ends the packet the sanitizer sees any that does not.
// (On the device resident packets sit in exact-size allocations too.)  A stand-alone program: tests/test_motion_fetch_emu.py compiles it (into its temporary directory), writes
// its packets to a file and runs it as a child process.
//   motion_fetch_asan FILE      FILE = { uint32 bytes, uint32 forms (bit 0: <true>, bit 1: <false>), the packet } ...
// Prints one line per packet and form with a sum of the records written; exit status 0 when every packet ran.
#include "pred_emu.cpp"

static int run(const uint8_t *pkt, bool has_l1, unsigned long idx)
{
	const E264FrameHdr *h = (const E264FrameHdr *)pkt;
	const size_t n = (size_t)h->width_mbs * h->height_mbs * E264_DBK_BYTES;
	uint8_t *out = (uint8_t *)malloc(n);
	memset(out, 0x5A, n);
	const int r = has_l1 ? emu_dbkparam<true>(pkt, out, nullptr) : emu_dbkparam<false>(pkt, out, nullptr);
	unsigned long sum = 0;
	for (size_t i = 0; i < n; i++) sum = sum * 31 + out[i];
	printf("packet %lu form %s: %d, %zu bytes, sum %lu\n", idx, has_l1 ? "<true>" : "<false>", r, n, sum);
	free(out);
	return r;
}

int main(int argc, char **argv)
{
	if (argc != 2) { fprintf(stderr, "usage: %s FILE\n", argv[0]); return 2; }
	FILE *f = fopen(argv[1], "rb");
	if (!f) { perror(argv[1]); return 2; }
	uint32_t head[2];
	unsigned long idx = 0;
	int bad = 0;
	while (fread(head, 4, 2, f) == 2) {
		uint8_t *pkt = (uint8_t *)malloc(head[0]); // exactly the packet: what follows it is not the program's
		if (head[0] < sizeof(E264FrameHdr) || fread(pkt, 1, head[0], f) != head[0]) { fprintf(stderr, "packet %lu: short file\n", idx); return 2; }
		if (((const E264FrameHdr *)pkt)->total_bytes != head[0]) { fprintf(stderr, "packet %lu: %u bytes in a block of %u\n", idx, ((const E264FrameHdr *)pkt)->total_bytes, head[0]); return 2; }
		if (head[1] & 1) bad |= run(pkt, true, idx);
		if (head[1] & 2) bad |= run(pkt, false, idx);
		free(pkt);
		idx++;
	}
	fclose(f);
	return bad ? 1 : 0;
}
