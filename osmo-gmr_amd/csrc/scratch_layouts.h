// scratch_layouts.h -- the blocks of device scratch of the host layer's kernel chains, each written once (scratch_carve.h):
// constructed on a null base a layout measures its block (`bytes`), constructed on the block it names the arrays the
// kernels' argument structs want.  Every block starts on a 128-byte boundary.  Host only, no HIP.
#pragma once

#include "scratch_carve.h"

#include "../../include/gmr1_hip.h"

namespace gmr1 {

// the TCH3 call follower over n frames (capi_tch3_follow.cpp), in the block's order: per-frame results, job slots,
// keystreams, and the decodes [0] plain and [1] deciphered
struct FollowScratch {
	int32_t *call, *p, *krv, *drv, *bt, *dsid, *frv, *fsid, *srv, *scv[2], *fcrc[2], *fcv[2];
	float *et, *en, *dtoa, *ftoa;
	int8_t *feb, *seb, *jeb;
	uint8_t *cls, *need, *kss, *ksf, *sfr[2], *fl[2];
	uint32_t *jfn;
	size_t bytes;
	FollowScratch(void *base, size_t n)
	{
		Carve c(base);
		call = c.take<int32_t>(n); p = c.take<int32_t>(n); et = c.take<float>(n); en = c.take<float>(n);
		krv = c.take<int32_t>(n); drv = c.take<int32_t>(n); bt = c.take<int32_t>(n); dsid = c.take<int32_t>(n);
		dtoa = c.take<float>(n); frv = c.take<int32_t>(n); fsid = c.take<int32_t>(n); ftoa = c.take<float>(n);
		srv = c.take<int32_t>(n); feb = c.take<int8_t>(n * 104); seb = c.take<int8_t>(n * 212);
		cls = c.take<uint8_t>(n); need = c.take<uint8_t>(n); jeb = c.take<int8_t>(n * 416); jfn = c.take<uint32_t>(n * 4);
		kss = c.take<uint8_t>(n * 208); ksf = c.take<uint8_t>(n * 384);
		for (int v = 0; v < 2; v++) sfr[v] = c.take<uint8_t>(n * 20);
		for (int v = 0; v < 2; v++) scv[v] = c.take<int32_t>(n * 2);
		for (int v = 0; v < 2; v++) fl[v] = c.take<uint8_t>(n * 10);
		for (int v = 0; v < 2; v++) fcrc[v] = c.take<int32_t>(n);
		for (int v = 0; v < 2; v++) fcv[v] = c.take<int32_t>(n);
		bytes = c.bytes();
	}
};
inline size_t tch3_follow_scratch_bytes(int n_frames) { return FollowScratch(nullptr, (size_t)n_frames).bytes; }

// the TCH9 call follower over n frames (capi_tch9_follow.cpp): the demodulator's outputs, the plan, keystreams, decodes
struct Follow9Scratch {
	int8_t *eb;
	int32_t *sid, *rv, *src, *call, *fcrc, *fcv, *tcv;
	uint8_t *cls, *need, *ks, *fl2, *tl2;
	size_t bytes;
	Follow9Scratch(void *base, size_t n)
	{
		Carve c(base);
		eb = c.take<int8_t>(n * 662); sid = c.take<int32_t>(n); rv = c.take<int32_t>(n);
		cls = c.take<uint8_t>(n); need = c.take<uint8_t>(n); src = c.take<int32_t>(n * 3); call = c.take<int32_t>(n);
		ks = c.take<uint8_t>(n * 658); fl2 = c.take<uint8_t>(n * 64); tl2 = c.take<uint8_t>(n * 64);
		fcrc = c.take<int32_t>(n); fcv = c.take<int32_t>(n); tcv = c.take<int32_t>(n);
		bytes = c.bytes();
	}
};
inline size_t tch9_follow_scratch_bytes(int n_frames) { return Follow9Scratch(nullptr, (size_t)n_frames).bytes; }

// the FCCH acquisition over n carriers of `peaks` candidate slots each (capi_fcch.cpp): [per carrier ... | per slot ...]
struct AcqScratch {
	uint64_t *base, *len, *off;
	int32_t *stat, *align, *base_align, *can3, *peaks, *toa1, *rv1, *ftoa, *count, *ctoa, *live;
	float *ferr, *fe, *cfe, *snr, *fs;
	size_t bytes;
	AcqScratch(void *block, size_t n, size_t n_peaks)
	{
		const size_t S = n * n_peaks;
		Carve c(block);
		base = c.take<uint64_t>(n); len = c.take<uint64_t>(n); stat = c.take<int32_t>(n); align = c.take<int32_t>(n);
		base_align = c.take<int32_t>(n); ferr = c.take<float>(n); can3 = c.take<int32_t>(n); off = c.take<uint64_t>(S);
		peaks = c.take<int32_t>(S); toa1 = c.take<int32_t>(n); rv1 = c.take<int32_t>(n); ftoa = c.take<int32_t>(n);
		fe = c.take<float>(n); count = c.take<int32_t>(n); ctoa = c.take<int32_t>(S); cfe = c.take<float>(S);
		snr = c.take<float>(S); live = c.take<int32_t>(S); fs = c.take<float>(S);
		bytes = c.bytes();
	}
};

// the audio close-up (capi_ambe.cpp): a slot per frame, a sink block per call
struct AudioScratch {
	int32_t *slot;
	gmr1_hip_rx_audio *sink;
	size_t bytes;
	AudioScratch(void *base, size_t n_calls, size_t n_frames)
	{
		Carve c(base);
		slot = c.take<int32_t>(n_frames); sink = c.take<gmr1_hip_rx_audio>(n_calls);
		bytes = c.bytes();
	}
};
inline size_t tch3_audio_scratch_bytes(int n_calls, int n_frames) { return AudioScratch(nullptr, n_calls, n_frames).bytes; }

// the receive loop's acquisition over A carriers (capi_rx.cpp), device block and pinned mirror: what goes up, what comes back
struct AcqBlock {
	uint64_t *offset, *length;
	gmr1_hip_fcch_acq *results;
	size_t up_bytes, bytes;
	AcqBlock(void *base, size_t A)
	{
		Carve c(base);
		offset = c.take<uint64_t>(A); length = c.take<uint64_t>(A);
		up_bytes = c.bytes();
		results = c.take<gmr1_hip_fcch_acq>(A);
		bytes = c.bytes();
	}
};

}  // namespace gmr1
