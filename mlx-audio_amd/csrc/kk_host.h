// Host-side plumbing shared by the runtimes (Kokoro kk_model.hip, CSM kk_csm.hip, Mimi kk_mimi.hip, Whisper kk_whisper.hip and
// kk_whisper_text.hip): parameter loaders, weight arena, graph replay cache, workspace bump allocator, debug notes and the error helpers.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "kk_kernels.h"

#define KK_TRY(x)                 \
  do {                            \
    const int rc__ = (x);         \
    if (rc__ != 0) return rc__;   \
  } while (0)

// kk_fail with a printf-style message
__attribute__((format(printf, 1, 2))) static inline int kk_failf(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  return kk_fail(buf);
}

static inline int rup(int v, int m) { return (v + m - 1) / m * m; }

// fp32 -> bf16 bits, round to nearest even
static inline uint16_t f32_to_bf16_rne(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x40);  // NaN stays NaN
  u += 0x7FFFu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

// hipMalloc + copy of a host staging vector on `st`, wait for it, then free the staging memory
template <typename T>
static inline int kk_upload(std::vector<T>& staging, T** dev, hipStream_t st, const char* who) {
  if (hipMalloc((void**)dev, staging.size() * sizeof(T)) != hipSuccess) return kk_failf("%s: hipMalloc failed", who);
  if (hipMemcpyAsync(*dev, staging.data(), staging.size() * sizeof(T), hipMemcpyHostToDevice, st) != hipSuccess)
    return kk_failf("%s: upload failed", who);
  if (hipStreamSynchronize(st) != hipSuccess) return kk_failf("%s: stream sync failed", who);
  std::vector<T>().swap(staging);
  return 0;
}

// ------------------------------------------------------------------------------------------------------------- weight arena
struct HostTensor {  // a loaded parameter, fp32, with the shape it was loaded with
  std::vector<float> d;
  std::vector<int64_t> shape;
};

// the body of a handle's *_load_tensor (`host`: its map, null for a null handle)
static inline int kk_host_load_tensor(const char* who, std::map<std::string, HostTensor>* host, bool finalized, const char* name, const int64_t* shape, int ndim,
                                      const float* data) {
  if (!host || !name || !shape || !data || ndim < 1) return kk_failf("%s: bad argument", who);
  if (finalized) return kk_failf("%s: model already finalized", who);
  size_t n = 1;
  for (int i = 0; i < ndim; ++i) n *= (size_t)shape[i];
  HostTensor& t = (*host)[name];
  t.d.assign(data, data + n);
  t.shape.assign(shape, shape + ndim);
  return 0;
}

// the loaded parameter `name` if it has `shape`, else null with the first such failure kept in `err`
static inline const HostTensor* kk_host_want(const std::map<std::string, HostTensor>& host, const std::string& name, std::initializer_list<int64_t> shape,
                                             std::string& err) {
  auto it = host.find(name);
  if (it == host.end()) {
    if (err.empty()) err = "missing parameter: " + name;
    return nullptr;
  }
  if (it->second.shape != std::vector<int64_t>(shape)) {
    if (err.empty()) err = "unexpected shape for " + name;
    return nullptr;
  }
  return &it->second;
}

// a quantised nn.Linear / nn.Embedding as an MLX checkpoint holds it (host, until finalize)
struct QuantHost {
  int O = 0, I = 0, group = 0, bits = 0;
  std::vector<uint32_t> words;        // [O][I * bits / 32]
  std::vector<float> scales, biases;  // [O][I / group]
};

// the body of a handle's *_load_quantized (`map`: its quantised tensors, null for a null handle)
static inline int kk_host_load_quantized(const char* who, std::map<std::string, QuantHost>* map, bool finalized, const char* name, const int64_t* shape,
                                         const uint32_t* words, const float* scales, const float* biases, int group_size, int bits) {
  if (!map || !name || !shape || !words || !scales || !biases) return kk_failf("%s: bad argument", who);
  if (finalized) return kk_failf("%s: model already finalized", who);
  if (bits != 2 && bits != 4 && bits != 8) return kk_failf("%s: bits must be 2, 4 or 8 (values of a word in bits [j bits, (j + 1) bits))", who);
  const int64_t O = shape[0], I = shape[1];
  if (O < 1 || I < 1 || O > (1 << 30) || I > (1 << 30) || group_size < 1 || I % group_size != 0 || (I * bits) % 32 != 0)
    return kk_failf("%s: %s: shape / group size", who, name);
  QuantHost& t = (*map)[name];
  t.O = (int)O; t.I = (int)I; t.group = group_size; t.bits = bits;
  t.words.assign(words, words + (size_t)O * (size_t)(I * bits / 32));
  t.scales.assign(scales, scales + (size_t)O * (size_t)(I / group_size));
  t.biases.assign(biases, biases + (size_t)O * (size_t)(I / group_size));
  return 0;
}

// the checkpoint's own arithmetic on the host: w = fp32(q) * scale + bias, two roundings (quant.dequantize_affine)
static inline void dequantize_host(const QuantHost& t, std::vector<float>& out) {
  const int per = 32 / t.bits, wpr = t.I / per, ngrp = t.I / t.group;
  const uint32_t mask = (1u << t.bits) - 1u;
  out.resize((size_t)t.O * t.I);
  for (int o = 0; o < t.O; ++o)
    for (int i = 0; i < t.I; ++i) {
      const float qf = (float)((t.words[(size_t)o * wpr + i / per] >> ((i % per) * t.bits)) & mask);
      volatile float prod = qf * t.scales[(size_t)o * ngrp + i / t.group];  // (rounded to fp32 before the add whatever the compiler's contraction rule)
      out[(size_t)o * t.I + i] = prod + t.biases[(size_t)o * ngrp + i / t.group];
    }
}

struct ArenaVec {  // n floats at `off` of the arena; `p` is set by resolve() after the upload
  size_t off = 0, n = 0;
  const float* p = nullptr;
};

// All packed fp32 parameters of a model in one host vector, uploaded as one device buffer.  Every block starts on a 64-float (256-byte)
// boundary.  alloc() may reallocate `pack`: take pointers into it only after the last alloc() they must survive.
struct WeightArena {
  std::map<std::string, HostTensor> host;  // parameters as loaded, by name (freed by upload)
  std::vector<float> pack;                 // host staging of the packed parameters (freed by upload)
  float* dev = nullptr;                    // device copy of `pack`; the owning model frees it
  std::string err;                         // the first "missing parameter" / "unexpected size" of get()

  size_t alloc(size_t n) {  // zero-filled
    const size_t off = (pack.size() + 63) & ~(size_t)63;
    pack.resize(off + n, 0.f);
    return off;
  }
  const HostTensor* get(const std::string& name, size_t n) {
    auto it = host.find(name);
    if (it == host.end()) {
      if (err.empty()) err = "missing parameter: " + name;
      return nullptr;
    }
    if (it->second.d.size() != n) {
      if (err.empty()) err = "unexpected size for " + name;
      return nullptr;
    }
    return &it->second;
  }
  ArenaVec put(const float* v, size_t n) {
    ArenaVec r;
    r.n = n;
    r.off = alloc(n);
    if (n) memcpy(&pack[r.off], v, n * 4);
    return r;
  }
  ArenaVec vec(const std::string& name, size_t n) {
    const HostTensor* t = get(name, n);
    return t ? put(t->d.data(), n) : ArenaVec();
  }
  int upload(hipStream_t st, const char* who) {
    KK_TRY(kk_upload(pack, &dev, st, who));
    host.clear();
    return 0;
  }
  void resolve(ArenaVec& v) const { v.p = v.n ? dev + v.off : nullptr; }
};

// ------------------------------------------------------------------------------------------------------------- graph replay cache
// One instantiated hipGraph per argument key, oldest dropped first beyond `capacity`.  First sight of a key runs the work eagerly (the
// one-time hipFuncSetAttribute calls of first launches must not land in a capture); the second captures it on a private stream (the
// caller's may be the legacy default stream, which cannot be captured; nothing runs during capture); from then on the caller launches
// the graph on its own stream.  clear() must run before the buffers a graph points at are freed.  A copy starts empty, so no graph
// handle is ever owned twice.
class GraphCache {
 public:
  explicit GraphCache(size_t capacity) : capacity_(capacity) {}
  GraphCache(const GraphCache& o) : capacity_(o.capacity_) {}
  GraphCache& operator=(const GraphCache&) = delete;
  ~GraphCache() {
    clear();
    if (cap_stream_) (void)hipStreamDestroy(cap_stream_);
  }

  void clear() {
    for (auto& e : entries_) destroy(e);
    entries_.clear();
  }

  // work(hipStream_t, bool capturing) -> 0 or an error.  Returns work's result on an eager run (*exec = null), else 0 with *exec set to the
  // graph for the caller to launch.  Error messages start with `who`.
  template <typename Work>
  int run(const std::vector<unsigned long long>& key, hipStream_t st, Work&& work, hipGraphExec_t* exec, const char* who) {
    *exec = nullptr;
    Entry* e = nullptr;
    for (auto& g : entries_)
      if (g.key == key) e = &g;
    if (!e) {
      if (entries_.size() >= capacity_) {
        destroy(entries_.front());
        entries_.erase(entries_.begin());
      }
      entries_.emplace_back();
      e = &entries_.back();
      e->key = key;
    }
    if (!e->seen) {
      e->seen = true;
      return work(st, false);
    }
    if (!e->exec) {
      if (!cap_stream_ && hipStreamCreateWithFlags(&cap_stream_, hipStreamNonBlocking) != hipSuccess)
        return kk_failf("%s: hipStreamCreate failed", who);
      if (hipStreamBeginCapture(cap_stream_, hipStreamCaptureModeThreadLocal) != hipSuccess)
        return kk_failf("%s: hipStreamBeginCapture failed", who);
      const int rc = work(cap_stream_, true);
      hipGraph_t g = nullptr;
      const hipError_t err = hipStreamEndCapture(cap_stream_, &g);
      if (rc != 0) {
        if (g) (void)hipGraphDestroy(g);
        return rc;
      }
      if (err != hipSuccess || !g) return kk_failf("%s: hipStreamEndCapture failed", who);
      hipGraphExec_t ex = nullptr;
      if (hipGraphInstantiate(&ex, g, nullptr, nullptr, 0) != hipSuccess) {
        (void)hipGraphDestroy(g);
        return kk_failf("%s: hipGraphInstantiate failed", who);
      }
      e->graph = g;
      e->exec = ex;
    }
    *exec = e->exec;
    return 0;
  }

 private:
  struct Entry {
    std::vector<unsigned long long> key;
    bool seen = false;  // ran eagerly once: first-launch attribute calls are done
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;  // set once captured
  };
  static void destroy(Entry& e) {
    if (e.exec) (void)hipGraphExecDestroy(e.exec);
    if (e.graph) (void)hipGraphDestroy(e.graph);
  }
  size_t capacity_;
  std::vector<Entry> entries_;
  hipStream_t cap_stream_ = nullptr;
};

// ------------------------------------------------------------------------------------------------------------- workspace
// Bump allocator over a caller's workspace, 256-byte aligned.  Without a base it only sizes (`used`); a dry run WITH a base hands out
// the same pointers as the real run (kk_forward_audio replays the text stage's plan this way).  Past `cap` it records `oom`.
struct Workspace {
  char* base = nullptr;
  size_t cap = 0, used = 0;
  bool dry = false, oom = false;
  void* raw(size_t bytes) {
    const size_t off = (used + 255) & ~(size_t)255;
    used = off + bytes;
    if (!base) return nullptr;
    if (used > cap) {
      oom = true;
      return nullptr;
    }
    return base + off;
  }
};

// ------------------------------------------------------------------------------------------------------------- debug notes
struct DebugNote {  // an intermediate of the last call: B items of rows x C valid channels at pitch ld, item stride bs (elements)
  const void* p;
  int ld;
  long long bs;
  int rows, C, dtype, B;
};

struct DebugNotes {
  std::map<std::string, DebugNote> map;
  int info(const char* who, const char* name, int64_t* rows, int64_t* channels) const {
    auto it = map.find(name);
    if (it == map.end()) return kk_failf("%s: no intermediate named %s in the last call", who, name);
    if (rows) *rows = it->second.rows;
    if (channels) *channels = it->second.C;
    return 0;
  }
  // any dtype / pitch -> dense fp32 [B][rows][C]
  int fetch(const char* who, const char* name, hipStream_t st, float* dst) const {
    auto it = map.find(name);
    if (it == map.end()) return kk_failf("%s: no intermediate named %s in the last call", who, name);
    const DebugNote& e = it->second;
    return kk_launch_convert(e.p, e.dtype, e.bs, e.ld, dst, KK_F32, (long long)e.rows * e.C, e.C, e.C, e.rows, e.B, st);
  }
};
