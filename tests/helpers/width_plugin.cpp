// A merge plugin templated over the k-mer width, the other kind kmtricks loads (use_template() = 1: one create<MAX_K>() per
// width of its KMER_LIST): it rebuilds each row's key as km::Kmer<MAX_K> and keeps the rows whose k-mer is its canonical form.
// Built by tests/test_tools_cpu.py against include/kmtricks alone.
#include <kmtricks/plugin.hpp>

template <size_t MAX_K>
class CanonicalRows : public km::IMergePlugin {
 public:
  bool process_kmer(const uint64_t* data, std::vector<count_type>&) override {
    km::Kmer<MAX_K> kmer(m_kmer_size);
    kmer.set64_p(data);
    return kmer == kmer.canonical();
  }
};

extern "C" std::string plugin_name() { return "CanonicalRows"; }
extern "C" int use_template() { return 1; }
extern "C" km::IMergePlugin* create32() { return new CanonicalRows<32>(); }
extern "C" km::IMergePlugin* create64() { return new CanonicalRows<64>(); }
extern "C" void destroy(km::IMergePlugin* p) { delete p; }
