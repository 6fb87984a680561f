// Host-side strided copies and a persistent worker pool.
//
// Reference: memcopy!/memcopy_threads! (src/update_halo.jl:755-774) copy flat
// halo buffers with Julia threads above GG_THREADCOPY_THRESHOLD bytes. Here the
// same threshold gates a persistent std::thread pool (no OpenMP runtime, so the
// library never fights PyTorch's libgomp for threads).
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <thread>

#include "igg/accum.hpp"
#include "igg/copy.hpp"

namespace igg {
namespace {

class Pool {
 public:
  Pool() {
    unsigned hw = std::thread::hardware_concurrency();
    if (const char* e = std::getenv("IGG_HOST_THREADS")) hw = static_cast<unsigned>(std::atoi(e));
    nworkers_ = std::max(1u, std::min(hw, 64u)) - 1;  // caller participates
    for (unsigned i = 0; i < nworkers_; ++i) threads_.emplace_back([this] { loop(); });
  }
  ~Pool() {
    {
      std::lock_guard<std::mutex> lk(m_);
      stop_ = true;
    }
    cv_.notify_all();
    for (auto& t : threads_) t.join();
  }
  unsigned size() const { return nworkers_ + 1; }

  void run(int64_t nchunks, const std::function<void(int64_t)>& body) {
    std::lock_guard<std::mutex> run_lock(run_m_);  // one parallel region at a time
    {
      std::lock_guard<std::mutex> lk(m_);
      body_ = &body;
      next_.store(0);
      nchunks_ = nchunks;
      pending_ = nworkers_;
      ++gen_;
    }
    cv_.notify_all();
    work();
    std::unique_lock<std::mutex> lk(m_);
    done_cv_.wait(lk, [this] { return pending_ == 0; });
    body_ = nullptr;
  }

 private:
  void work() {
    for (;;) {
      int64_t c = next_.fetch_add(1);
      if (c >= nchunks_) break;
      (*body_)(c);
    }
  }
  void loop() {
    uint64_t seen = 0;
    for (;;) {
      {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
        if (stop_) return;
        seen = gen_;
      }
      work();
      {
        std::lock_guard<std::mutex> lk(m_);
        if (--pending_ == 0) done_cv_.notify_one();
      }
    }
  }

  unsigned nworkers_ = 0;
  std::vector<std::thread> threads_;
  std::mutex m_, run_m_;
  std::condition_variable cv_, done_cv_;
  const std::function<void(int64_t)>* body_ = nullptr;
  std::atomic<int64_t> next_{0};
  int64_t nchunks_ = 0;
  unsigned pending_ = 0;
  uint64_t gen_ = 0;
  bool stop_ = false;
};

Pool& pool() {
  static Pool p;
  return p;
}

template <typename T>
void copy_rows(const Copy2D& c, int64_t o0, int64_t o1) {
  const T* src = reinterpret_cast<const T*>(c.src);
  T* dst = reinterpret_cast<T*>(c.dst);
  const size_t row_bytes = static_cast<size_t>(c.n_inner) * sizeof(T);
  for (int64_t o = o0; o < o1; ++o) {
    const T* s = src + o * c.src_so;
    T* d = dst + o * c.dst_so;
    if (c.src_si == 1 && c.dst_si == 1) {
      std::memcpy(d, s, row_bytes);
    } else {
      for (int64_t i = 0; i < c.n_inner; ++i) d[i * c.dst_si] = s[i * c.src_si];
    }
  }
}

struct alignas(16) B16 { uint64_t x, y; };

void copy_range(const Copy2D& c, int eb, int64_t o0, int64_t o1) {
  switch (eb) {
    case 1: copy_rows<uint8_t>(c, o0, o1); break;
    case 2: copy_rows<uint16_t>(c, o0, o1); break;
    case 4: copy_rows<uint32_t>(c, o0, o1); break;
    case 8: copy_rows<uint64_t>(c, o0, o1); break;
    case 16: copy_rows<B16>(c, o0, o1); break;
    default: fail("host_copy2d: unsupported element size ", eb, " bytes");
  }
}

}  // namespace

void host_parallel_for(int64_t n, int64_t grain, const std::function<void(int64_t, int64_t)>& fn) {
  if (n <= 0) return;
  grain = std::max<int64_t>(1, grain);
  const int64_t nchunks = (n + grain - 1) / grain;
  if (nchunks == 1 || pool().size() == 1) { fn(0, n); return; }
  std::function<void(int64_t)> body = [&](int64_t ch) {
    fn(ch * grain, std::min(n, (ch + 1) * grain));
  };
  pool().run(nchunks, body);
}

void host_copy2d(const std::vector<Copy2D>& copies, int elem_bytes) {
  for (const Copy2D& c : copies) {
    const int64_t bytes = c.n_outer * c.n_inner * elem_bytes;
    if (bytes <= 0) continue;
    if (bytes < THREADCOPY_THRESHOLD || c.n_outer < 2) {
      copy_range(c, elem_bytes, 0, c.n_outer);
    } else {
      const int64_t rows_per_chunk =
          std::max<int64_t>(1, c.n_outer / (4 * static_cast<int64_t>(pool().size())));
      host_parallel_for(c.n_outer, rows_per_chunk,
                        [&](int64_t o0, int64_t o1) { copy_range(c, elem_bytes, o0, o1); });
    }
  }
}

void host_copy3d(const std::vector<Copy3D>& copies, int elem_bytes) {
  // A slab is n_outer independent 2-D copies of n_mid rows; they run through
  // the 2-D path one after the other (each is threaded by its own size).
  std::vector<Copy2D> planes;
  for (const Copy3D& c : copies) {
    if (c.n_outer * c.n_mid * c.n_inner <= 0) continue;
    for (int64_t o = 0; o < c.n_outer; ++o)
      planes.push_back({c.src + o * c.src_so * elem_bytes, c.dst + o * c.dst_so * elem_bytes, c.n_mid,
                        c.n_inner, c.src_sm, c.src_si, c.dst_sm, c.dst_si});
  }
  host_copy2d(planes, elem_bytes);
}

// ---------------------------------------------------------------- accumulation
//
// Host equivalent of accum3d_batch_kernel (igg/accum.hpp): the reference the
// GPU result is compared with bit for bit, and the data path of
// accumulate_halo_ for CPU fields. Half and bfloat16 add the way torch does on
// the CPU: in float, rounded once to the storage type.
namespace {

struct Half { uint16_t bits; };
struct BFloat { uint16_t bits; };

inline float to_float(BFloat v) {
  const uint32_t u = static_cast<uint32_t>(v.bits) << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
inline BFloat to_bfloat(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return {static_cast<uint16_t>(0x7fc0u)};  // NaN
  u += 0x7fffu + ((u >> 16) & 1u);  // to nearest, ties to even
  return {static_cast<uint16_t>(u >> 16)};
}
inline float to_float(Half v) {
  const uint32_t s = static_cast<uint32_t>(v.bits & 0x8000u) << 16;
  uint32_t e = (v.bits >> 10) & 0x1fu, m = v.bits & 0x3ffu, u;
  if (e == 0 && m == 0) {
    u = s;
  } else if (e == 0) {  // subnormal: normal in float
    e = 113;
    while (!(m & 0x400u)) m <<= 1, --e;
    u = s | (e << 23) | ((m & 0x3ffu) << 13);
  } else if (e == 31) {
    u = s | 0x7f800000u | (m << 13);
  } else {
    u = s | ((e + 112) << 23) | (m << 13);
  }
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
inline Half to_half(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  const uint16_t s = static_cast<uint16_t>((u >> 16) & 0x8000u);
  u &= 0x7fffffffu;
  if (u > 0x7f800000u) return {static_cast<uint16_t>(s | 0x7e00u)};   // NaN
  if (u >= 0x47800000u) return {static_cast<uint16_t>(s | 0x7c00u)};  // >= 2^16 (and inf): inf
  if (u < 0x33000000u) return {s};                                    // < 2^-25: zero
  const uint32_t e = u >> 23;
  uint32_t m = (u & 0x7fffffu) | 0x800000u;  // 24 significant bits
  // bits to drop: 13 for a normal half (e >= 113), more for a subnormal one
  const uint32_t drop = e >= 113 ? 13 : 13 + (113 - e);
  const uint32_t half = 1u << (drop - 1), rest = m & ((1u << drop) - 1);
  m >>= drop;
  if (rest > half || (rest == half && (m & 1u))) ++m;  // to nearest, ties to even
  // (a carry out of the mantissa moves into the exponent field, as it must)
  const uint32_t h = e >= 113 ? ((e - 113) << 10) + m : m;  // (m holds the implicit bit of a normal half)
  return {static_cast<uint16_t>(s | h)};
}

struct C64 { float re, im; };
struct C128 { double re, im; };

template <typename T>
inline T add_elem(T a, T b) { return static_cast<T>(a + b); }
template <>
inline C64 add_elem(C64 a, C64 b) { return {a.re + b.re, a.im + b.im}; }
template <>
inline C128 add_elem(C128 a, C128 b) { return {a.re + b.re, a.im + b.im}; }
template <>
inline Half add_elem(Half a, Half b) { return to_half(to_float(a) + to_float(b)); }
template <>
inline BFloat add_elem(BFloat a, BFloat b) { return to_bfloat(to_float(a) + to_float(b)); }
// (integers wrap, as torch's do)
template <>
inline int8_t add_elem(int8_t a, int8_t b) { return static_cast<int8_t>(static_cast<uint8_t>(a) + static_cast<uint8_t>(b)); }
template <>
inline int16_t add_elem(int16_t a, int16_t b) { return static_cast<int16_t>(static_cast<uint16_t>(a) + static_cast<uint16_t>(b)); }
template <>
inline int32_t add_elem(int32_t a, int32_t b) { return static_cast<int32_t>(static_cast<uint32_t>(a) + static_cast<uint32_t>(b)); }
template <>
inline int64_t add_elem(int64_t a, int64_t b) { return static_cast<int64_t>(static_cast<uint64_t>(a) + static_cast<uint64_t>(b)); }

template <typename T>
void accum_rows(const Accum3D& a, int64_t r0, int64_t r1) {
  const Copy3D& c = a.c;
  T* src = reinterpret_cast<T*>(const_cast<char*>(c.src));
  T* dst = reinterpret_cast<T*>(c.dst);
  const bool adds = static_cast<int>(a.op) & 1, takes = static_cast<int>(a.op) & 2, zero = a.op == AccumOp::Zero;
  T nought;
  std::memset(&nought, 0, sizeof(T));  // +0 of every type
  for (int64_t r = r0; r < r1; ++r) {
    const int64_t o = r / c.n_mid, m = r - o * c.n_mid;
    T* s = src + o * c.src_so + m * c.src_sm;
    T* d = dst + o * c.dst_so + m * c.dst_sm;
    for (int64_t i = 0; i < c.n_inner; ++i) {
      T& dv = d[i * c.dst_si];
      if (zero) {
        dv = nought;
        continue;
      }
      T& sv = s[i * c.src_si];
      dv = adds ? add_elem<T>(dv, sv) : sv;
      if (takes) sv = nought;
    }
  }
}

template <typename T>
void accum_typed(const Accum3D& a) {
  const Copy3D& c = a.c;
  const int64_t rows = c.n_outer * c.n_mid;
  if (rows <= 0 || c.n_inner <= 0) return;
  const int64_t bytes = rows * c.n_inner * static_cast<int64_t>(sizeof(T));
  if (bytes < THREADCOPY_THRESHOLD || rows < 2) return accum_rows<T>(a, 0, rows);
  const int64_t grain = std::max<int64_t>(1, rows / (4 * static_cast<int64_t>(pool().size())));
  host_parallel_for(rows, grain, [&](int64_t r0, int64_t r1) { accum_rows<T>(a, r0, r1); });
}

}  // namespace

void host_accum3d(const std::vector<Accum3D>& ops, AccumType type) {
  for (const Accum3D& a : ops) {
    switch (type) {
      case AccumType::F32: accum_typed<float>(a); break;
      case AccumType::F64: accum_typed<double>(a); break;
      case AccumType::I8: accum_typed<int8_t>(a); break;
      case AccumType::I16: accum_typed<int16_t>(a); break;
      case AccumType::I32: accum_typed<int32_t>(a); break;
      case AccumType::I64: accum_typed<int64_t>(a); break;
      case AccumType::U8: accum_typed<uint8_t>(a); break;
      case AccumType::F16: accum_typed<Half>(a); break;
      case AccumType::BF16: accum_typed<BFloat>(a); break;
      case AccumType::C64: accum_typed<C64>(a); break;
      case AccumType::C128: accum_typed<C128>(a); break;
      default: fail("host_accum3d: unknown element type ", static_cast<int>(type));
    }
  }
}

}  // namespace igg
