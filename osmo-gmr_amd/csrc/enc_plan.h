// enc_plan.h -- the position map of one encoder chain as k_encode reads it (tx_kernels.hip), the chains there are, and the
// host function that writes a chain's map down (enc_plan.cpp: plain host arithmetic over l1_codes.h, no HIP).
// capi_encode.cpp uploads a plan once per chain and device; tests/c/enc_plan_host.cpp checks every field of every plan.
#pragma once
#include <cstdint>

namespace gmr1 {

constexpr int kEncMaxIn = 64;          // payload bytes of one unit (TCH9 9k6: 60)
constexpr int kEncMaxExt = 512;        // bits of the extended information word (TCH9 9k6: 480 + 8)
constexpr int kEncMaxOut = 672;        // burst bits of one unit (NT9: 662)
struct EncPlan {
	int32_t n_in0, n_in1;              // payload bytes per unit: first / second input array
	int32_t n_ext;                     // extended information word: [K-1 preset bits | info + CRC | flush zeros] ...
	int32_t n_out;                     // burst bits written per unit
	int32_t n_aux0, n_aux1;            // multiplexed-in bits per unit (status / SACCH): first / second array
	int32_t n_ciph;                    // keystream bits per unit
	int32_t depth;                     // 1, or 3: inter-burst interleaver (bursts n, n-1, n-2 of a run)
	uint32_t poly[8];                  // window masks over K consecutive bits of the extended word
	uint16_t crc_tab[kEncMaxIn * 8];   // what payload bit b adds to CRC register A (the CRCs are linear: init 0, no final xor)
	uint16_t crc_tab2[kEncMaxIn * 8];  // the same for CRC register B (RACH: CRC12), else zeros
	uint16_t ext_src[kEncMaxExt];      // where every bit of the extended word comes from (see tx_kernels.hip)
	uint32_t out[kEncMaxOut];          // descriptor of every burst bit (see tx_kernels.hip)
};

// the chains; the order is the ABI of gmr1_hip_encoder_plan and of api.ENC_CHAINS
enum PlanId { kPlBcch = 0, kPlCcch, kPlFacch3, kPlTch3M0, kPlTch3M1, kPlFacch9, kPlTch9_2k4, kPlTch9_4k8, kPlTch9_9k6,
              kPlRach, kPlXch, kPlCount };

// the plan of chain `id` (a PlanId), every byte of *out written
#pragma GCC visibility push(hidden)
void build_enc_plan(int id, EncPlan *out);
#pragma GCC visibility pop

}  // namespace gmr1
