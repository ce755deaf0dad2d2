/*
 * forged_check.c - the oracle's decoders on a corpus of forged streams, as a program of its
 * own linked with AddressSanitizer + UBSan (make forged).  TEST INFRASTRUCTURE ONLY.
 *
 *   forged_check <corpus> <huffman table>
 *
 * Corpus: "FRG1", u32 count, then per case u32 method id, u32 room, u32 length and the
 * stream's bytes (little endian, tests/_forge.py writes it).  Every stream is copied into a
 * malloc block of exactly its length and decoded into a block of exactly `room` samples, so a
 * read or a write outside either is a finding.  One line per case: index, po_depress's return
 * value, out_n and the FNV-1a sum of the decoded samples' bytes (0 0 for a refused read).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "press_oracle.c"

static int rd32(FILE *f, uint32_t *v)
{
	uint8_t b[4];
	if (fread(b, 1, 4, f) != 4)
		return -1;
	*v = get_u32(b);
	return 0;
}

int main(int argc, char **argv)
{
	FILE *f;
	uint32_t count, k;
	char magic[4];
	if (argc != 3) {
		fprintf(stderr, "usage: forged_check <corpus> <huffman table>\n");
		return 2;
	}
	if (po_load_table(argv[2])) {
		fprintf(stderr, "cannot load %s\n", argv[2]);
		return 2;
	}
	f = fopen(argv[1], "rb");
	if (!f || fread(magic, 1, 4, f) != 4 || memcmp(magic, "FRG1", 4) || rd32(f, &count)) {
		fprintf(stderr, "cannot read %s\n", argv[1]);
		return 2;
	}
	for (k = 0; k < count; k++) {
		uint32_t method, room, len, out_n = 0, h = 0x811C9DC5u, i;
		uint8_t *in;
		int16_t *out;
		int ret;
		if (rd32(f, &method) || rd32(f, &room) || rd32(f, &len)) {
			fprintf(stderr, "case %u: short corpus\n", k);
			return 2;
		}
		in = malloc(len);
		out = malloc((size_t) room * sizeof *out);
		if ((len && !in) || (room && !out) || fread(in, 1, len, f) != len) {
			fprintf(stderr, "case %u: short corpus\n", k);
			return 2;
		}
		ret = po_depress((int) method, in, len, room, out, &out_n);
		if (ret) {
			out_n = 0;
			h = 0;
		} else {
			const uint8_t *b = (const uint8_t *) out;
			for (i = 0; i < 2 * out_n; i++)
				h = (h ^ b[i]) * 0x01000193u;
		}
		printf("%u %d %u %u\n", k, ret, out_n, h);
		free(in);
		free(out);
	}
	fclose(f);
	return 0;
}
