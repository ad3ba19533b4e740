// The per-device cache without HIP (osmo-gmr_amd/csrc/dev_cache.h): eight threads, each acting as one of eight devices, ask
// for the eleven keys in an order of their own, several times over -- 88 entries, what a process that encodes every chain on
// every device of an eight-GPU box makes.  make runs once per (device, key); the address handed out first is the one handed
// out ever after, and still holds what make wrote after all 88 inserts; a make that fails leaves nothing behind.  Run plain,
// under the address and undefined-behaviour sanitizers and under the thread sanitizer by tests/test_dev_cache_host.py (nothing
// is preloaded).
#include <atomic>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "dev_cache.h"

using namespace gmr1;

namespace {

constexpr int kDevices = 8, kKeys = 11, kRounds = 5;

struct Entry {
	int device, key;
	unsigned char body[5824];          // an encoder plan's size: a few entries fill a deque's block
};

DevCache<int, Entry> g_cache;
std::atomic<int> g_makes{0}, g_ready{0}, g_bad{0};
const Entry *g_first[kDevices][kKeys];

void bad(const char *what, int device, int key)
{
	std::printf("device %d key %d: %s\n", device, key, what);
	g_bad++;
}

unsigned char mark(int device, int key) { return (unsigned char)(1 + 16 * device + key); }

bool whole(const Entry *e, int device, int key)
{
	if (e->device != device || e->key != key)
		return false;
	for (unsigned char b : e->body)
		if (b != mark(device, key))
			return false;
	return true;
}

void worker(int device)
{
	g_ready++;
	while (g_ready.load() < kDevices)
		std::this_thread::yield();
	for (int round = 0; round < kRounds; round++)
		for (int i = 0; i < kKeys; i++) {
			const int key = (device * 3 + i * (round % 2 ? 7 : 4) + round) % kKeys;      // 4 and 7 are coprime to 11
			const Entry *e = nullptr;
			const int r = g_cache.get(device, key, &e, [&](Entry *n) {
				g_makes++;
				n->device = device;
				n->key = key;
				std::memset(n->body, mark(device, key), sizeof(n->body));
				return 0;
			});
			if (r || !e) {
				bad("get failed", device, key);
				continue;
			}
			if (!g_first[device][key])
				g_first[device][key] = e;      // (a row of g_first belongs to one thread)
			else if (g_first[device][key] != e)
				bad("the address changed", device, key);
			if (!whole(e, device, key))
				bad("the entry does not hold what make wrote", device, key);
		}
}

}  // namespace

int main()
{
	std::vector<std::thread> ts;
	for (int d = 0; d < kDevices; d++)
		ts.emplace_back(worker, d);
	for (std::thread &t : ts)
		t.join();
	if (g_makes.load() != kDevices * kKeys) {
		std::printf("make ran %d times, not %d\n", g_makes.load(), kDevices * kKeys);
		g_bad++;
	}
	// after all 88 inserts: every first address still answers, and still holds its contents
	for (int d = 0; d < kDevices; d++)
		for (int k = 0; k < kKeys; k++) {
			const Entry *e = nullptr;
			const int r = g_cache.get(d, k, &e, [&](Entry *) { g_makes++; return -1; });
			if (r || e != g_first[d][k] || !e || !whole(e, d, k))
				bad("lost after the last insert", d, k);
		}
	// a make that fails: its code comes back, no entry stays, the next get makes again; the one that succeeds is kept
	int calls = 0;
	const Entry *e = nullptr;
	for (int i = 0; i < 2; i++)
		if (g_cache.get(3, 99, &e, [&](Entry *) { calls++; return -5; }) != -5 || e)
			bad("a failing make did not come back as its code", 3, 99);
	if (calls != 2)
		bad("a failed make left an entry behind", 3, 99);
	auto good = [&](Entry *n) { calls++; n->device = 3; n->key = 99; std::memset(n->body, mark(3, 99), sizeof(n->body)); return 0; };
	const Entry *e2 = nullptr;
	if (g_cache.get(3, 99, &e, good) || g_cache.get(3, 99, &e2, good) || calls != 3 || !e || e != e2 || !whole(e, 3, 99))
		bad("the make after a failed one was not run once and kept", 3, 99);
	if (g_makes.load() != kDevices * kKeys)
		bad("a hit ran make", -1, -1);
	if (g_bad.load()) {
		std::printf("%d checks failed\n", g_bad.load());
		return 1;
	}
	std::printf("ok\n");
	return 0;
}
