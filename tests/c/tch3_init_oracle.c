/* The oracle's rx_tch3_init (oracle/orc_rx.c, static there) behind a flat interface, for tests/test_rx_stream_tch_host.py:
 * this file includes the oracle's translation unit and is linked against liborc.so for everything else. */
#include "orc_rx.c"

struct tch3_flat {      /* struct gmr1_hip_tch3_state up to its key */
	int32_t active, p, ciph, weak_cnt, sync_id, burst_cnt;
	float energy_dkab, energy_burst;
	uint32_t bi_fn[4];
	int8_t ebits[416];
};

/* IMMEDIATE ASSIGNMENT with timeslot tn and DKAB position p -> rx_tch3_init on *f; returns the timeslot it parsed */
int tch3_init_oracle(struct tch3_flat *f, int tn, int p, float ref_energy)
{
	struct chan_desc cd;
	struct tch3_state *st = &cd.tch3_state;
	uint8_t l2[24];
	memset(&cd, 0, sizeof(cd));
	memset(l2, 0, sizeof(l2));
	l2[1] = 0x06;
	l2[2] = 0x3f;
	l2[8] = (uint8_t)((p << 2) | (tn >> 3));
	l2[9] = (uint8_t)((tn & 7) << 5);
	st->active = f->active; st->p = f->p; st->ciph = f->ciph; st->weak_cnt = f->weak_cnt;
	st->sync_id = f->sync_id; st->burst_cnt = f->burst_cnt;
	st->energy_dkab = f->energy_dkab; st->energy_burst = f->energy_burst;
	memcpy(st->bi_fn, f->bi_fn, sizeof(f->bi_fn));
	memcpy(st->ebits, f->ebits, sizeof(f->ebits));
	if (!ccch_is_imm_ass(l2))
		return -1;
	rx_tch3_init(&cd, l2, ref_energy);
	f->active = st->active; f->p = st->p; f->ciph = st->ciph; f->weak_cnt = st->weak_cnt;
	f->sync_id = st->sync_id; f->burst_cnt = st->burst_cnt;
	f->energy_dkab = st->energy_dkab; f->energy_burst = st->energy_burst;
	memcpy(f->bi_fn, st->bi_fn, sizeof(f->bi_fn));
	memcpy(f->ebits, st->ebits, sizeof(f->ebits));
	return st->tn;
}
