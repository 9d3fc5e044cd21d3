// The NF4 table of the 4-bit frozen decoder base (QLoRA, --bits 4 --quant_type nf4), as fp32 bit patterns: THE device-side definition
// of the format (tests/nf4_ref.py TABLE states the sixteen values in decimal; tests/test_nf4_host.py holds the two equal).
// Ascending, code 0 = -1.0, code 7 = 0.0, code 15 = 1.0.  The second level of double quantisation uses rv_adam8_signed_bits of
// adam8_codebook.h.  radvlm_amd/nf4.py reads this file too (the hash trainer_state.json records): keep one 0x???????? word per entry.
#pragma once
#include <stdint.h>
#ifndef RV_NF4_TABLE
#define RV_NF4_TABLE static const
#endif
RV_NF4_TABLE uint32_t rv_nf4_bits[16] = {
    0xbf800000, 0xbf3239b1, 0xbf066b30, 0xbeca32a0, 0xbe91a24d, 0xbe3d353f, 0xbdba7871, 0x00000000,
    0x3da2faff, 0x3e24cae3, 0x3e7c04dd, 0x3ead033a, 0x3ee1a4b8, 0x3f1007ab, 0x3f3913b3, 0x3f800000,
};
