// rx_touch.h -- where a wave touches the NEXT burst's window while it works on this one (rx_window.h: window_touch_q).
// Plain arithmetic, no device code: a host program can include this file alone and check every address.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GMR1_TOUCH_HD __host__ __device__
#else
#define GMR1_TOUCH_HD
#endif

namespace gmr1 {

static constexpr int kTouchLine = 128;            // bytes of a cache line
// A window of at most 1024 samples of 8 bytes that does not start on a line overlaps 65 lines: slot 0 is the window's first
// dword, slot k >= 1 the first dword of the k-th line behind the one the window starts in.  Lane l takes slot l, lane 0
// slot 64 as well.
static constexpr int kTouchSlots = 65;

// Is burst g + 1 touched while burst g = g0 + q of a wave is worked on?  Only a burst the same wave takes next.
GMR1_TOUCH_HD inline bool window_touch_wanted(int q, int g, int n_end)
{
	return q < 3 && g + 1 < n_end;
}

// Byte offset, counted from the window's first byte, of the dword touch `slot` reads; -1: this slot reads nothing.
// misalign: the first byte's address modulo the line (a multiple of 8: the samples are float2); in_len: samples in the window.
// Every offset lies in [0, 8 in_len - 4], and the slots that read cover every line the window's bytes overlap.
GMR1_TOUCH_HD inline int window_touch_offset(unsigned misalign, int in_len, int slot)
{
	if (slot < 0 || slot >= kTouchSlots || in_len <= 0)
		return -1;
	const int last = 8 * in_len - 4;              // the window's last dword
	const int o = slot == 0 ? 0 : kTouchLine * slot - (int)(misalign & (unsigned)(kTouchLine - 1));
	return o <= last ? o : -1;
}

}  // namespace gmr1
