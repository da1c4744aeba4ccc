// tools/record_width_probe.hip -- what the access width is worth for the particle position streams on MI355X: the four 4-byte
// arrays key, t[0], t[1], t[2] (one dword per lane and memory instruction) against one 16-byte record {key, t[3]} per particle,
// at 2^26 elements, in the two patterns the step has:
//  (a) coalesced, shaped like k_advect_collide_count: 8 particles per lane 64 apart, every load issued before the first value is
//      used and before any store; with and without the three 4-byte velocity streams that the advection reads beside them;
//  (b) scattered, shaped like k_tile_scatter and the correction's epilogue: lane i stores to slot p(i), p a random permutation
//      inside consecutive windows of 3800 slots (a C4 tile); the values come from registers alone (store only) or from a coalesced
//      read of the same layout (the tile scatter).
// The variants of a pattern alternate launch by launch; each line is the median, fastest and slowest of REPS launches in GB/s of
// algorithmic bytes. A sample of every destination is checked on the host.
// build: hipcc --offload-arch=gfx950 -O3 -o tools/record_width_probe tools/record_width_probe.hip ; run once on the GPU box under
// a time limit: timeout -k 10 120 tools/record_width_probe
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>

#define CHUNKS 8  // particles per lane, as AC_CHUNKS in particles.hip
#define WINDOW 3800
#define REPS 15

struct Rec {
	uint32_t key;
	float t[3];
};
static_assert(sizeof(Rec) == 16, "one record is one 16-byte access");

struct Streams {
	uint32_t *key;
	float *t[3];
};

#define CHECK(x)                                                                                       \
	do {                                                                                               \
		hipError_t e_ = (x);                                                                           \
		if (e_ != hipSuccess) {                                                                        \
			fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));         \
			exit(2);                                                                                   \
		}                                                                                              \
	} while (0)

__device__ inline Rec load_rec(const Rec *a, size_t i) {
	const uint4 q = *(const uint4 *)(a + i);
	Rec r;
	r.key = q.x;
	r.t[0] = __uint_as_float(q.y); r.t[1] = __uint_as_float(q.z); r.t[2] = __uint_as_float(q.w);
	return r;
}
__device__ inline void store_rec(Rec *a, size_t i, const Rec &r) {
	*(uint4 *)(a + i) = make_uint4(r.key, __float_as_uint(r.t[0]), __float_as_uint(r.t[1]), __float_as_uint(r.t[2]));
}
__device__ inline Rec load_streams(const Streams &s, size_t i) {
	Rec r;
	r.key = s.key[i];
#pragma unroll
	for (int d = 0; d < 3; ++d) r.t[d] = s.t[d][i];
	return r;
}
__device__ inline void store_streams(const Streams &s, size_t i, const Rec &r) {
	s.key[i] = r.key;
#pragma unroll
	for (int d = 0; d < 3; ++d) s.t[d][i] = r.t[d];
}
/// a little arithmetic between load and store, so that the copy cannot be folded into wider moves
__device__ inline void touch(Rec &r, float vx, float vy, float vz) {
	r.key += 1u;
	r.t[0] += vx; r.t[1] += vy; r.t[2] += vz;
}
/// the value particle i carries in the store-only scatter
__host__ __device__ inline Rec rec_of(uint32_t i) {
	Rec r;
	r.key = i;
	r.t[0] = (float)(i & 1023u); r.t[1] = (float)(i >> 10 & 1023u); r.t[2] = (float)(i >> 20);
	return r;
}

/// (a): in place, as the advection. n is a multiple of 64 * CHUNKS * (256 / 64); the index is clamped all the same.
template <bool REC, bool VEL>
__global__ void __launch_bounds__(256) k_coalesced(size_t n, Rec *rec, Streams s, const float *v0, const float *v1, const float *v2) {
	const int lane = threadIdx.x & 63;
	const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
	const size_t i0 = wave * (64 * CHUNKS) + lane;
	Rec r[CHUNKS];
	float v[CHUNKS][3];
#pragma unroll
	for (int c = 0; c < CHUNKS; ++c) {
		const size_t i = i0 + 64 * c < n ? i0 + 64 * c : n - 1;
		r[c] = REC ? load_rec(rec, i) : load_streams(s, i);
		v[c][0] = VEL ? v0[i] : 1.0f; v[c][1] = VEL ? v1[i] : 2.0f; v[c][2] = VEL ? v2[i] : 3.0f;
	}
#pragma unroll
	for (int c = 0; c < CHUNKS; ++c) touch(r[c], v[c][0], v[c][1], v[c][2]);
#pragma unroll
	for (int c = 0; c < CHUNKS; ++c) {
		const size_t i = i0 + 64 * c;
		if (i >= n) continue;
		if (REC) store_rec(rec, i, r[c]);
		else store_streams(s, i, r[c]);
	}
}

/// (b): lane i stores to slot p[i] < n (checked on the host before the upload). READ: the value is read from src in the same
/// layout, else it is rec_of(i).
template <bool REC, bool READ>
__global__ void __launch_bounds__(256) k_scatter(size_t n, const uint32_t *p, const Rec *src_rec, Streams src, Rec *dst_rec, Streams dst) {
	const int lane = threadIdx.x & 63;
	const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
	const size_t i0 = wave * (64 * CHUNKS) + lane;
	Rec r[CHUNKS];
	uint32_t to[CHUNKS];
#pragma unroll
	for (int c = 0; c < CHUNKS; ++c) {
		const size_t i = i0 + 64 * c < n ? i0 + 64 * c : n - 1;
		to[c] = p[i];
		if (READ) r[c] = REC ? load_rec(src_rec, i) : load_streams(src, i);
		else r[c] = rec_of((uint32_t)i);
	}
#pragma unroll
	for (int c = 0; c < CHUNKS; ++c) {
		if (i0 + 64 * c >= n) continue;
		if (REC) store_rec(dst_rec, to[c], r[c]);
		else store_streams(dst, to[c], r[c]);
	}
}

struct Stat {
	const char *name;
	double bytes;
	std::vector<float> ms;
};
static void report(Stat &s) {
	std::sort(s.ms.begin(), s.ms.end());
	const double med = s.ms[s.ms.size() / 2], lo = s.ms.front(), hi = s.ms.back();
	printf("  %-44s %8.1f us  median %7.1f GB/s  (fastest %7.1f, slowest %7.1f)\n", s.name, 1e3 * med, s.bytes / med * 1e-6,
	       s.bytes / lo * 1e-6, s.bytes / hi * 1e-6);
}

static Streams alloc_streams(size_t n) {
	Streams s;
	CHECK(hipMalloc(&s.key, n * 4)); CHECK(hipMemset(s.key, 0, n * 4));
	for (int d = 0; d < 3; ++d) { CHECK(hipMalloc(&s.t[d], n * 4)); CHECK(hipMemset(s.t[d], 0, n * 4)); }
	return s;
}

int main() {
	const size_t n = (size_t)1 << 26;
	const int grid = (int)(n / (256 * CHUNKS));
	// p: a Fisher-Yates shuffle (64-bit LCG) inside every window of WINDOW consecutive slots; the last window is the short one
	std::vector<uint32_t> p(n);
	uint64_t x = 0x853c49e6748fea9bull;
	for (size_t w = 0; w < n; w += WINDOW) {
		const size_t m = std::min<size_t>(WINDOW, n - w);
		for (size_t k = 0; k < m; ++k) p[w + k] = (uint32_t)(w + k);
		for (size_t k = m - 1; k > 0; --k) {
			x = x * 6364136223846793005ull + 1442695040888963407ull;
			std::swap(p[w + k], p[w + (size_t)((x >> 33) % (k + 1))]);
		}
	}
	for (size_t i = 0; i < n; ++i)
		if (p[i] >= n || p[i] / WINDOW != i / WINDOW) { fprintf(stderr, "p[%zu] = %u leaves its window\n", i, p[i]); return 2; }

	uint32_t *dp;
	CHECK(hipMalloc(&dp, n * 4)); CHECK(hipMemcpy(dp, p.data(), n * 4, hipMemcpyHostToDevice));
	Rec *rec[2];
	Streams st[2];
	for (int k = 0; k < 2; ++k) {
		CHECK(hipMalloc(&rec[k], n * sizeof(Rec))); CHECK(hipMemset(rec[k], 0, n * sizeof(Rec)));
		st[k] = alloc_streams(n);
	}
	float *v[3];
	for (int d = 0; d < 3; ++d) { CHECK(hipMalloc(&v[d], n * 4)); CHECK(hipMemset(v[d], 0, n * 4)); }
	hipEvent_t e0, e1;
	CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
	const double N = (double)n;

	Stat a[4] = {{"4 x 4 B in place", 32 * N, {}}, {"1 x 16 B in place", 32 * N, {}},
	             {"4 x 4 B in place + 3 velocity streams read", 44 * N, {}}, {"1 x 16 B in place + 3 velocity streams read", 44 * N, {}}};
	Stat b[4] = {{"store only, 4 x 4 B into four arrays", 20 * N, {}}, {"store only, 1 x 16 B into one array", 20 * N, {}},
	             {"read coalesced + store, 4 x 4 B", 36 * N, {}}, {"read coalesced + store, 1 x 16 B", 36 * N, {}}};
	for (int rep = -2; rep < REPS; ++rep) {  // two warm-up rounds
		for (int k = 0; k < 8; ++k) {
			CHECK(hipEventRecord(e0));
			switch (k) {
			case 0: hipLaunchKernelGGL((k_coalesced<false, false>), dim3(grid), dim3(256), 0, 0, n, rec[0], st[0], v[0], v[1], v[2]); break;
			case 1: hipLaunchKernelGGL((k_coalesced<true, false>), dim3(grid), dim3(256), 0, 0, n, rec[0], st[0], v[0], v[1], v[2]); break;
			case 2: hipLaunchKernelGGL((k_coalesced<false, true>), dim3(grid), dim3(256), 0, 0, n, rec[0], st[0], v[0], v[1], v[2]); break;
			case 3: hipLaunchKernelGGL((k_coalesced<true, true>), dim3(grid), dim3(256), 0, 0, n, rec[0], st[0], v[0], v[1], v[2]); break;
			case 4: hipLaunchKernelGGL((k_scatter<false, false>), dim3(grid), dim3(256), 0, 0, n, dp, rec[0], st[0], rec[1], st[1]); break;
			case 5: hipLaunchKernelGGL((k_scatter<true, false>), dim3(grid), dim3(256), 0, 0, n, dp, rec[0], st[0], rec[1], st[1]); break;
			case 6: hipLaunchKernelGGL((k_scatter<false, true>), dim3(grid), dim3(256), 0, 0, n, dp, rec[0], st[0], rec[1], st[1]); break;
			case 7: hipLaunchKernelGGL((k_scatter<true, true>), dim3(grid), dim3(256), 0, 0, n, dp, rec[0], st[0], rec[1], st[1]); break;
			}
			CHECK(hipGetLastError());
			CHECK(hipEventRecord(e1));
			CHECK(hipEventSynchronize(e1));
			float ms = 0;
			CHECK(hipEventElapsedTime(&ms, e0, e1));
			if (rep >= 0) (k < 4 ? a[k] : b[k - 4]).ms.push_back(ms);
		}
	}
	printf("record width probe: %zu elements, %d per lane, %d launches each, alternating\n", n, CHUNKS, REPS);
	printf("(a) coalesced, all loads before the first store\n");
	for (Stat &s : a) report(s);
	printf("(b) scattered inside windows of %d slots\n", WINDOW);
	for (Stat &s : b) report(s);

	// the reading scatters wrote rec[1] / st[1] last: run the store-only pair once more and check what it leaves
	hipLaunchKernelGGL((k_scatter<false, false>), dim3(grid), dim3(256), 0, 0, n, dp, rec[0], st[0], rec[1], st[1]);
	hipLaunchKernelGGL((k_scatter<true, false>), dim3(grid), dim3(256), 0, 0, n, dp, rec[0], st[0], rec[1], st[1]);
	CHECK(hipDeviceSynchronize());
	const size_t m = (size_t)1 << 20;  // the first 2^20 slots and the last
	std::vector<Rec> hr(m), hr2(m);
	std::vector<uint32_t> hk(m), hk2(m);
	std::vector<float> ht(m), ht2(m);
	CHECK(hipMemcpy(hr.data(), rec[1], m * sizeof(Rec), hipMemcpyDeviceToHost));
	CHECK(hipMemcpy(hr2.data(), rec[1] + (n - m), m * sizeof(Rec), hipMemcpyDeviceToHost));
	CHECK(hipMemcpy(hk.data(), st[1].key, m * 4, hipMemcpyDeviceToHost));
	CHECK(hipMemcpy(hk2.data(), st[1].key + (n - m), m * 4, hipMemcpyDeviceToHost));
	CHECK(hipMemcpy(ht.data(), st[1].t[2], m * 4, hipMemcpyDeviceToHost));
	CHECK(hipMemcpy(ht2.data(), st[1].t[2] + (n - m), m * 4, hipMemcpyDeviceToHost));
	std::vector<uint32_t> inv(n);
	for (size_t i = 0; i < n; ++i) inv[p[i]] = (uint32_t)i;
	size_t bad = 0;
	for (size_t j = 0; j < m; ++j) {
		const Rec lo = rec_of(inv[j]), hi = rec_of(inv[n - m + j]);
		bad += hr[j].key != lo.key || hr[j].t[0] != lo.t[0] || hr[j].t[1] != lo.t[1] || hr[j].t[2] != lo.t[2];
		bad += hr2[j].key != hi.key || hr2[j].t[0] != hi.t[0] || hr2[j].t[1] != hi.t[1] || hr2[j].t[2] != hi.t[2];
		bad += hk[j] != lo.key || hk2[j] != hi.key || ht[j] != lo.t[2] || ht2[j] != hi.t[2];
	}
	printf("check of 2 x %zu scattered slots per layout: %zu wrong\n", m, bad);
	return bad ? 1 : 0;
}
