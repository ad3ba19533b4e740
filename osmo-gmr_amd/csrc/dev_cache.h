// dev_cache.h -- what is made once per (device, key) and kept: the encoder plans, the modulator's tables, the NT9 gather maps,
// the channelizer's plans.  Host code without HIP (the caller asks hipGetDevice and passes the index in), so
// tests/c/dev_cache_host.cpp runs it from eight threads on its own.
#pragma once
#include <deque>
#include <mutex>

#pragma GCC visibility push(hidden)
namespace gmr1 {

template <class Key, class Entry> class DevCache {
public:
	// the entry of (device, key); on a miss make(&entry) builds it under the lock.  Addresses stay valid for the life
	// of the process (a deque).  A make that fails leaves no entry behind, and the next get tries again.
	template <class Make> int get(int device, const Key &key, const Entry **out, Make &&make)
	{
		std::lock_guard<std::mutex> lk(mu_);
		for (const Slot &s : slots_)
			if (s.device == device && s.key == key) {
				*out = &s.entry;
				return 0;
			}
		slots_.push_back(Slot{device, key, Entry()});
		const int r = make(&slots_.back().entry);
		if (r) {
			slots_.pop_back();
			return r;
		}
		*out = &slots_.back().entry;
		return 0;
	}

private:
	struct Slot { int device; Key key; Entry entry; };
	std::mutex mu_;
	std::deque<Slot> slots_;
};

}  // namespace gmr1
#pragma GCC visibility pop
