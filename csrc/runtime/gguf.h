// Native GGUF v2/v3 parser over a read-only mmap.
// Tensor payloads are never copied at parse time: `data(name)` is a pointer
// into the mapping, streamed to the GPU (after the planar repack) at load.
#pragma once
#include <cstdint>
#include <map>
#include <memory>
#include <string>
#include <vector>

namespace lfk {

struct GGUFValue {
  enum Kind { NONE, INT, FLOAT, BOOL, STRING, ARR_INT, ARR_FLOAT, ARR_STRING, ARR_BOOL } kind = NONE;
  int64_t i = 0;
  double f = 0;
  bool b = false;
  std::string s;
  std::vector<int64_t> ai;
  std::vector<double> af;
  std::vector<std::string> as;
};

struct GGUFTensor {
  std::string name;
  int type = 0;
  std::vector<int64_t> ne;  // ggml order: ne[0] innermost
  uint64_t offset = 0;      // absolute file offset
  uint64_t nbytes = 0;
  int64_t n_elements() const {
    int64_t n = 1;
    for (auto d : ne) n *= d;
    return n;
  }
};

class GGUFFile {
 public:
  explicit GGUFFile(const std::string& path);
  ~GGUFFile();
  GGUFFile(const GGUFFile&) = delete;
  GGUFFile& operator=(const GGUFFile&) = delete;

  const std::map<std::string, GGUFValue>& metadata() const { return kv_; }
  const std::vector<GGUFTensor>& tensors() const { return tensors_; }
  const GGUFTensor* find(const std::string& name) const;
  const uint8_t* data(const GGUFTensor& t) const { return base_ + t.offset; }
  bool has(const std::string& key) const { return kv_.count(key) > 0; }
  int64_t get_int(const std::string& key, int64_t dflt) const;
  double get_float(const std::string& key, double dflt) const;
  std::string get_str(const std::string& key, const std::string& dflt) const;
  uint32_t version() const { return version_; }
  size_t file_size() const { return size_; }
  // advise the kernel to read ahead a tensor's pages (overlaps disk IO with the repack)
  void prefetch(const GGUFTensor& t) const;

 private:
  void parse();  // header, KV pairs and tensor infos of the mapped file (throws on malformed input)

  std::string path_;
  int fd_ = -1;
  const uint8_t* base_ = nullptr;
  size_t size_ = 0;
  uint32_t version_ = 0;
  std::map<std::string, GGUFValue> kv_;
  std::vector<GGUFTensor> tensors_;
  std::map<std::string, size_t> index_;
};

// Model hyper-parameters as the GPU engine and the CPU backend read them from the metadata
// (general.architecture llama / mistral / mixtral / qwen2 / qwen3; anything else is refused). qwen3:
// head_dim is qwen3.attention.key_length where present (it need not be n_embd / n_head), 64 or 128.
struct HParams {
  int n_vocab = 0, n_embd = 0, n_layer = 0, n_head = 0, n_head_kv = 0, head_dim = 0, n_ff = 0;
  int n_expert = 0, n_expert_used = 0, n_ctx_train = 0;
  float rope_base = 10000.f, rms_eps = 1e-5f;
  std::string arch = "llama";
  // NeoX RoPE pairs (i, i + head_dim / 2): the loaders permute the rows of attn_q / attn_k inside
  // each head (neox_src_row) so that every kernel keeps rotating adjacent pairs
  bool rope_neox = false;
  // blk.N.attn_{q,k,v}.bias (F32) are present: added to the projections before RoPE
  bool qkv_bias = false;
  // blk.N.attn_{q,k}_norm.weight (F32 [head_dim]) are present (qwen3): an RMSNorm over each q and k
  // head after the projection and before RoPE. The loaders permute these weights with the map of
  // the q / k rows (neox_src_row), which leaves a head's mean square as it was
  bool qk_norm = false;
  // {arch}.pooling_type (embedding models: 0 none, 1 mean, 2 cls, 3 last, 4 rank); -1: the key is absent
  int pooling_type = -1;
};
HParams read_hparams(const GGUFFile& f);

// NeoX -> adjacent-pair row order inside a head: row 2i of the permuted projection is row i of
// the file's, row 2i + 1 is row i + hd / 2 (`r` any row index of a matrix of whole heads)
inline size_t neox_src_row(size_t r, size_t hd) {
  const size_t j = r % hd;
  return r - j + (j >> 1) + ((j & 1) ? hd / 2 : 0);
}

}  // namespace lfk
