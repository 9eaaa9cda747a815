// pybind11 module `tensorframes_amd._C`: graph import/analysis, the executor,
// pinned host memory. Replaces the Py4J + JNI bridges of the reference
// (reference: src/main/scala/org/tensorframes/impl/PythonInterface.scala:21-180).
#include <torch/extension.h>

#include <unordered_map>
#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPGuard.h>

#include "comm/comm.h"
#include "ir/graph.h"
#include "kernels/kernels.h"
#include "runtime/device_pool.h"
#include "runtime/executor.h"
#include "runtime/fusion.h"
#include "runtime/jit.h"
#include "runtime/jpeg_decode.h"
#include "runtime/unpack.h"
#include <rocprofiler-sdk-roctx/roctx.h>

namespace py = pybind11;
using namespace tfa;

namespace tfa {
void register_packer(py::module& m);  // runtime/packer.cpp
void register_pyencode(py::module& m);  // proto/pyencode.cpp
}

namespace {

py::object shape_to_py(const Shape& s) {
  if (s.unknown_rank) return py::none();
  py::list l;
  for (auto d : s.dims) l.append(d);
  return l;
}

Shape shape_from_py(const py::object& o) {
  if (o.is_none()) return Shape::unknown();
  std::vector<int64_t> d;
  for (auto v : o) d.push_back(v.is_none() ? -1 : v.cast<int64_t>());
  return Shape(d);
}

const char* row_name(RowClass r) {
  switch (r) {
    case RowClass::CONST: return "const";
    case RowClass::ROW: return "row";
    default: return "mixed";
  }
}

// {name: (dtype_enum, dims|None)} -> TensorInfo map
std::map<std::string, TensorInfo> infos_from_py(const py::dict& d) {
  std::map<std::string, TensorInfo> m;
  for (auto kv : d) {
    auto t = kv.second.cast<py::tuple>();
    TensorInfo ti;
    ti.dtype = static_cast<DType>(t[0].cast<int>());
    ti.shape = shape_from_py(t[1]);
    m[kv.first.cast<std::string>()] = ti;
  }
  return m;
}

py::list infos_to_py(const std::vector<TensorInfo>& v) {
  py::list l;
  for (auto& ti : v) {
    py::dict d;
    d["dtype"] = static_cast<int>(ti.dtype);
    d["shape"] = shape_to_py(ti.shape);
    d["row"] = row_name(ti.row);
    d["const"] = ti.value.has_value();
    l.append(d);
  }
  return l;
}

// Static inference over every node of a graph (used by the DSL for
// get_shape()). Nodes that fail inference report an error string.
py::dict infer_all(const std::string& bytes) {
  auto g = Graph::from_bytes(bytes);
  std::vector<TensorRef> all;
  for (size_t i = 0; i < g->nodes().size(); ++i) all.push_back({static_cast<int>(i), 0});
  auto order = g->closure(all);
  Graph::Infos infos = g->infer(order, {}, false);
  py::dict out;
  for (size_t i = 0; i < g->nodes().size(); ++i) out[py::str(g->node(i).name)] = infos_to_py(infos[i]);
  return out;
}

// order-preserving integer image of float keys, the host twin of
// key_image in kernels/groupby.hip: NaNs -> one canonical NaN (sorted last),
// -0.0 -> +0.0, negative values' magnitude bits flipped
template <typename F, typename S>
at::Tensor key_image_typed(const at::Tensor& keys, at::ScalarType st) {
  at::Tensor out = pool_empty({keys.size(0)}, keys.options().dtype(st));
  const F* in = keys.data_ptr<F>();
  S* o = out.data_ptr<S>();
  const S flip = std::numeric_limits<S>::max();
  for (int64_t i = 0; i < keys.size(0); ++i) {
    F v = in[i];
    if (v != v) v = std::numeric_limits<F>::quiet_NaN();
    if (v == F(0)) v = F(0);
    S b;
    std::memcpy(&b, &v, sizeof(b));
    o[i] = b < 0 ? S(b ^ flip) : b;
  }
  return out;
}

template <typename F, typename S>
at::Tensor key_from_image_typed(const at::Tensor& img, at::ScalarType st) {
  at::Tensor out = pool_empty({img.size(0)}, img.options().dtype(st));
  const S* in = img.data_ptr<S>();
  F* o = out.data_ptr<F>();
  const S flip = std::numeric_limits<S>::max();
  for (int64_t i = 0; i < img.size(0); ++i) {
    S b = in[i] < 0 ? S(in[i] ^ flip) : in[i];
    std::memcpy(&o[i], &b, sizeof(b));
  }
  return out;
}

at::Tensor host_key_image(const at::Tensor& keys) {
  return keys.scalar_type() == at::kDouble ? key_image_typed<double, int64_t>(keys, at::kLong)
                                           : key_image_typed<float, int32_t>(keys, at::kInt);
}

at::Tensor host_key_from_image(const at::Tensor& img, at::ScalarType st) {
  return st == at::kDouble ? key_from_image_typed<double, int64_t>(img, st) : key_from_image_typed<float, int32_t>(img, st);
}

// the position of s in names, -1 when it is none of them
template <size_t N>
int name_index(const char* const (&names)[N], const std::string& s) {
  for (size_t i = 0; i < N; ++i)
    if (s == names[i]) return static_cast<int>(i);
  return -1;
}

// st is one of the seven statistics dtypes, or a type_error "<subject><st><object>, which is not supported (...)"
void require_stat_type(at::ScalarType st, const std::string& subject, const char* object) {
  if (st != at::kFloat && st != at::kDouble && st != at::kLong && st != at::kInt && st != at::kShort &&
      st != at::kChar && st != at::kByte)
    throw py::type_error(str_cat(subject, c10::toString(st), object, ", which is not supported (uint8, int8, int16, "
                                 "int32, int64, float32 or float64)"));
}

// a dense scalar column of one of the seven statistics dtypes, or the typed error
void stat_column(const char* what, const at::Tensor& t, const std::string& which) {
  if (!t.is_cuda()) throw py::value_error(str_cat(what, ": ", which, " must be a device tensor"));
  if (t.dim() != 1) throw py::value_error(str_cat(what, ": ", which, " must be 1-D (one scalar per row)"));
  require_stat_type(t.scalar_type(), str_cat(what, ": ", which, " is "), "");
  if (!t.is_contiguous())
    throw py::value_error(str_cat(what, ": ", which, " is not contiguous; make it contiguous first"));
}

// stat_column on the device and with the row count of `like` (ref names it in the errors)
void stat_column_like(const char* what, const at::Tensor& t, const std::string& which, const char* ref,
                      const at::Device& dev, int64_t n, DType* dtype, const void** ptr) {
  stat_column(what, t, which);
  if (t.device() != dev) throw py::value_error(str_cat(what, ": ", which, " is not on ", ref, "'s device"));
  if (t.size(0) != n) throw py::value_error(str_cat(what, ": ", which, " has ", t.size(0), " rows, ", ref, " ", n));
  *dtype = from_scalar_type(t.scalar_type());
  *ptr = t.data_ptr();
}

// 1..kMaxPackCols columns as on cols[0]'s device and with its row count
k::StatCols stat_cols_from(const char* what, const std::vector<at::Tensor>& cols) {
  if (cols.empty() || cols.size() > static_cast<size_t>(k::kMaxPackCols))
    throw py::value_error(str_cat(what, ": 1..", k::kMaxPackCols, " columns per call, got ", cols.size()));
  k::StatCols sc;
  sc.n = static_cast<int>(cols.size());
  stat_column(what, cols[0], "column 0");  // (before its row count is read)
  for (size_t c = 0; c < cols.size(); ++c)
    stat_column_like(what, cols[c], str_cat("column ", c), "the first column", cols[0].device(), cols[0].size(0),
                     &sc.dtype[c], &sc.ptr[c]);
  return sc;
}

}  // namespace

namespace tfa {
namespace k {
void set_conv_smallc(int on);  // kernels/conv_smallc.hip
void set_conv_direct(int on);  // kernels/conv_direct.hip
}  // namespace k
void set_pool_conv_fusion(bool on);  // runtime/executor.cpp
}  // namespace tfa

static thread_local int g_sort_last_passes = 0;  // radix passes of this thread's last sort_argsort

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "tensorframes_amd native runtime (GraphDef executor + HIP/CDNA4 kernels)";

  py::register_exception<GraphError>(m, "GraphError", PyExc_ValueError);
  py::register_exception<comm::CollectiveError>(m, "CollectiveError", PyExc_RuntimeError);

  py::class_<Graph, std::shared_ptr<Graph>>(m, "Graph")
      .def(py::init([](py::bytes b) { return Graph::from_bytes(std::string(b)); }))
      .def("structure_key", [](const Graph& g) { return g.structure_key(); },
           "hash of the graph without its parameter constants' payloads (Graph::structure_key)")
      .def("parameter_consts",
           [](const Graph& g) {
             std::vector<std::string> v;
             const auto& p = g.parameter_consts();
             for (size_t i = 0; i < p.size(); ++i)
               if (p[i]) v.push_back(g.node(static_cast<int>(i)).name);
             return v;
           })
      .def("node_names",
           [](const Graph& g) {
             std::vector<std::string> v;
             for (auto& n : g.nodes()) v.push_back(n.name);
             return v;
           })
      .def("node_ops",
           [](const Graph& g) {
             std::vector<std::string> v;
             for (auto& n : g.nodes()) v.push_back(n.op);
             return v;
           })
      .def("node_inputs",
           [](const Graph& g, const std::string& name) {
             int i = g.find(name);
             TFA_CHECK(i >= 0, "no node named '", name, "'");
             return g.def().nodes[i].inputs;
           })
      .def("placeholders",
           [](const Graph& g) {
             std::vector<std::string> v;
             for (int i : g.placeholders()) v.push_back(g.node(i).name);
             return v;
           })
      .def("zero_input_nodes",
           [](const Graph& g) {
             std::vector<std::string> v;
             for (auto& n : g.nodes())
               if (n.inputs.empty() && n.control.empty()) v.push_back(n.name);
             return v;
           })
      .def("has_node", [](const Graph& g, const std::string& n) { return g.find(n) >= 0; })
      .def("node_attr_scalars",
           [](const Graph& g, const std::string& name) {
             // scalar attrs (i / f / b / type / s) of one node, no tensors
             int i = g.find(name);
             TFA_CHECK(i >= 0, "no node named '", name, "'");
             py::dict d;
             for (auto& kv : g.def().nodes[i].attr) {
               const AttrValue& a = kv.second;
               switch (a.kind) {
                 case AttrValue::I: d[py::str(kv.first)] = a.i; break;
                 case AttrValue::F: d[py::str(kv.first)] = a.f; break;
                 case AttrValue::B: d[py::str(kv.first)] = a.b; break;
                 case AttrValue::TYPE: d[py::str(kv.first)] = static_cast<int>(a.type); break;
                 case AttrValue::S: d[py::str(kv.first)] = py::bytes(a.s); break;
                 default: break;
               }
             }
             return d;
           })
      .def("const_strings",
           [](const Graph& g, const std::string& name) {
             int i = g.find(name);
             TFA_CHECK(i >= 0, "no node named '", name, "'");
             const NodeDef& nd = g.def().nodes[i];
             py::list l;
             const AttrValue* v = nd.find_attr("value");
             if (nd.op == "Const" && v && v->tensor && v->tensor->dtype == DType::STRING)
               for (auto& str : v->tensor->strings) l.append(py::bytes(str));
             return l;
           })
      .def("serialize", [](const Graph& g) { return py::bytes(serialize_graphdef(g.def())); })
      .def("__len__", [](const Graph& g) { return g.nodes().size(); });

  py::class_<Program, std::shared_ptr<Program>>(m, "Program")
      .def(py::init([](std::shared_ptr<Graph> g, std::vector<std::string> fetches,
                       std::vector<std::string> feeds) {
             return std::make_shared<Program>(g, fetches, feeds);
           }),
           py::arg("graph"), py::arg("fetches"), py::arg("feeds"))
      .def_property_readonly("fetch_names", &Program::fetch_names)
      .def_property_readonly("feed_names", &Program::feed_names)
      .def("row_separable",
           [](const Program& p, py::dict hints) { return p.row_separable(infos_from_py(hints)); })
      .def("rebind", &Program::rebind, py::arg("values"), py::call_guard<py::gil_scoped_release>(),
           "a program with new parameter-constant payloads that takes over this one's plans")
      .def("adopt", &Program::adopt, py::arg("old"), py::call_guard<py::gil_scoped_release>(),
           "take over the plans of a structurally equal program (see executor.h)")
      .def("monoids",
           [](const Program& p) {
             py::list l;
             for (auto& mi : p.monoids()) l.append(py::make_tuple(mi.fetch, mi.placeholder, mi.op));
             return l;
           })
      .def("run", &Program::run, py::call_guard<py::gil_scoped_release>())
      .def("run_concurrent", &Program::run_concurrent, py::arg("inputs_list"), py::arg("max_streams") = 4,
           py::call_guard<py::gil_scoped_release>(),
           "independent runs over several input sets on one GPU, forked onto engine side streams and joined "
           "back into the caller's stream")
      .def("run_chunked", &Program::run_chunked, py::arg("seg_inputs"), py::arg("seg_outputs"),
           py::arg("chunk_rows"), py::arg("device"), py::arg("depth") = 3, py::arg("wait") = true,
           py::call_guard<py::gil_scoped_release>())
      .def("release_pipeline", &Program::release_pipeline, py::call_guard<py::gil_scoped_release>(),
           "drain and free the persistent chunk pipeline (after a deferred run_chunked sequence)")
      .def("run_chunked_reduce", &Program::run_chunked_reduce, py::arg("seg_inputs"), py::arg("chunk_rows"),
           py::arg("device"), py::arg("depth") = 3, py::call_guard<py::gil_scoped_release>())
      .def("describe", &Program::describe_plan, py::arg("inputs"), py::arg("as_gpu") = false)
      .def("fused_sources", &Program::fused_sources)
      .def("reset_stats", &Program::reset_stats)
      .def("stats", [](const Program& p) {
        ExecStats s = p.stats();
        py::dict d;
        d["runs"] = s.runs;
        d["kernels"] = s.kernels;
        d["plans_built"] = s.plans_built;
        d["plans_adopted"] = s.plans_adopted;
        d["h2d_bytes"] = s.h2d_bytes;
        d["d2h_bytes"] = s.d2h_bytes;
        d["d2h_dense_bytes"] = s.d2h_dense_bytes;  // what the D2H copies delivered (packed fetches expanded)
        d["chunks"] = s.chunks;
        d["chunks_packed"] = s.chunks_packed;
        d["wall_ms"] = s.wall_ms;
        d["plan_ms"] = s.plan_ms;
        d["exec_ms"] = s.exec_ms;
        d["h2d_ms"] = s.h2d_ms;        // device time of the host->device copies (hipEvents)
        d["compute_ms"] = s.compute_ms;
        d["d2h_ms"] = s.d2h_ms;
        d["graphs_captured"] = s.graphs_captured;
        d["graph_replays"] = s.graph_replays;
        d["graph_failures"] = s.graph_failures;
        d["graphs_declined"] = s.graphs_declined;
        d["graph_busy"] = s.graph_busy;
        return d;
      });

  m.def("analyze_fetches",
        [](std::shared_ptr<Graph> g, std::vector<std::string> fetches, std::vector<std::string> feeds,
           py::dict hints) {
          Program p(g, fetches, feeds);
          Graph::Infos infos = p.analyze(infos_from_py(hints));
          py::dict out;
          // per fetch and per feed: info of output 0 (or the indexed output)
          auto info_of = [&](const std::string& f) -> py::object {
            TensorRef r = g->resolve(f);
            TFA_CHECK(r.index < static_cast<int>(infos[r.node].size()), "tensor '", f,
                      "' does not exist (node has ", infos[r.node].size(), " outputs)");
            py::list l = infos_to_py({infos[r.node][r.index]});
            return py::object(l[0]);
          };
          for (auto& f : fetches) out[py::str(f)] = info_of(f);
          for (auto& f : feeds) out[py::str(f)] = info_of(f);
          return out;
        });
  m.def("infer_fed",
        [](std::shared_ptr<Graph> g, std::vector<std::string> fetches, std::vector<std::string> feeds,
           py::dict hints) {
          // per-node infos of a program's closure under concrete feed infos
          // (the map_rows vectorizer needs every tensor's rank)
          Program p(g, fetches, feeds);
          Graph::Infos infos = p.analyze(infos_from_py(hints));
          py::dict out;
          for (size_t i = 0; i < infos.size(); ++i)
            if (!infos[i].empty()) out[py::str(g->node(static_cast<int>(i)).name)] = infos_to_py(infos[i]);
          return out;
        });
  m.def("infer_all", &infer_all);
  // A GraphDef whose Const nodes above `max_elems` elements are replaced by
  // same-typed Placeholders: structure-only views of big models for
  // Python-side graph analysis (weights never cross into Python).
  m.def("light_graphdef", [](py::bytes b, int64_t max_elems) {
    GraphDef g = parse_graphdef(std::string(b));
    for (auto& nd : g.nodes) {
      if (nd.op != "Const") continue;
      const AttrValue* v = nd.find_attr("value");
      if (!v || !v->tensor || v->tensor->num_elements() <= max_elems) continue;
      AttrValue dt;
      dt.kind = AttrValue::TYPE;
      dt.type = v->tensor->dtype;
      AttrValue shp;
      shp.kind = AttrValue::SHAPE;
      shp.shape = v->tensor->shape;
      nd.op = "Placeholder";
      nd.attr.clear();
      nd.attr["dtype"] = dt;
      nd.attr["shape"] = shp;
    }
    return py::bytes(serialize_graphdef(g));
  });
  // `orig` with every node of `patch` replacing the same-named node (or
  // appended when new): applies a Python-side rewrite of a light view back
  // onto the full graph.
  m.def("patch_graphdef", [](py::bytes orig, py::bytes patch) {
    GraphDef g = parse_graphdef(std::string(orig));
    GraphDef p = parse_graphdef(std::string(patch));
    std::unordered_map<std::string, size_t> at;
    for (size_t i = 0; i < g.nodes.size(); ++i) at[g.nodes[i].name] = i;
    for (auto& nd : p.nodes) {
      auto it = at.find(nd.name);
      if (it != at.end()) g.nodes[it->second] = nd;
      else g.nodes.push_back(nd);
    }
    return py::bytes(serialize_graphdef(g));
  });
  m.def("registered_ops", [] { return OpRegistry::get().names(); });
  // float32 MatMul/Conv2D compute mode: 0 exact f32, 1 bf16, 2 bf16x3 (kernels/gemm_bf16.hip)
  m.def("set_f32_precision", [](int mode) { k::set_f32_precision(mode); });
  // device groupBy segmentation (kernels/groupby.hip); host tensors use the ATen oracle
  m.def("factorize", [](const at::Tensor& keys0) {
    TFA_CHECK(keys0.dim() == 1, "factorize: keys must be 1-D");
    at::Tensor keys = keys0.contiguous();
    const int64_t n = keys.size(0);
    if (!keys.is_cuda()) {
      // float keys through their order image (groupby.hip): every NaN is one
      // key sorted last, -0.0 and 0.0 are one key
      const bool fl = keys.scalar_type() == at::kFloat || keys.scalar_type() == at::kDouble;
      at::Tensor img = fl ? host_key_image(keys) : keys;
      auto r = at::_unique2(img, /*sorted=*/true, /*return_inverse=*/true, /*return_counts=*/false);
      at::Tensor uniq = fl ? host_key_from_image(std::get<0>(r), keys.scalar_type()) : std::get<0>(r);
      return py::make_tuple(std::get<1>(r).to(at::kLong), uniq);
    }
    c10::hip::HIPGuard guard(keys.device().index());
    auto opts = keys.options();
    if (n == 0) return py::make_tuple(pool_empty({0}, opts.dtype(at::kLong)), pool_empty({0}, opts));
    hipStream_t s = c10::hip::getCurrentHIPStream(keys.device().index()).stream();
    const DType dt = from_scalar_type(keys.scalar_type());
    const size_t wsb = k::factorize_workspace_bytes(dt, n);
    at::Tensor ws = pool_empty({static_cast<int64_t>(wsb)}, opts.dtype(at::kByte));
    at::Tensor ids = pool_empty({n}, opts.dtype(at::kLong));
    at::Tensor uniq = pool_empty({n}, opts);
    int64_t nseg = 0;
    {
      py::gil_scoped_release nogil;
      nseg = k::factorize(dt, keys.data_ptr(), n, ids.data_ptr<int64_t>(), uniq.data_ptr(), ws.data_ptr(), wsb, s);
    }
    return py::make_tuple(ids, uniq.narrow(0, 0, nseg));
  }, "keys [n] -> (group id per row int64, distinct keys ascending)");
  m.def("string_words", [](const at::Tensor& offsets, const at::Tensor& data, int64_t W) {
    TFA_CHECK(offsets.scalar_type() == at::kLong && offsets.dim() == 1 && offsets.size(0) >= 1,
              "string_words: offsets must be int64[n+1]");
    TFA_CHECK(data.scalar_type() == at::kByte && data.dim() == 1, "string_words: data must be uint8[bytes]");
    TFA_CHECK(W >= 1 && W <= 4096, "string_words: 1..4096 words");
    TFA_CHECK(offsets.device() == data.device(), "string_words: offsets and data on different devices");
    const int64_t n = offsets.size(0) - 1;
    at::Tensor oc = offsets.contiguous(), dc = data.contiguous();
    if (!oc.is_cuda()) {  // host: the same packing, a plain loop
      at::Tensor out = at::empty({W + 1, n}, oc.options());
      const int64_t* o = oc.data_ptr<int64_t>();
      const uint8_t* d = dc.data_ptr<uint8_t>();
      int64_t* y = out.data_ptr<int64_t>();
      for (int64_t i = 0; i < n; ++i) {
        const int64_t a = o[i], len = o[i + 1] - a;
        for (int64_t w = 0; w < W; ++w) {
          uint64_t v = 0;
          for (int b = 0; b < 8; ++b) {
            const int64_t j = w * 8 + b;
            v |= static_cast<uint64_t>(j < len ? d[a + j] : 0) << (56 - 8 * b);
          }
          y[w * n + i] = static_cast<int64_t>(v ^ 0x8000000000000000ull);
        }
        y[W * n + i] = len;
      }
      return out;
    }
    c10::hip::HIPGuard guard(oc.device().index());
    at::Tensor out = pool_empty({W + 1, n}, oc.options());
    k::string_words(oc.data_ptr<int64_t>(), dc.data_ptr<uint8_t>(), n, static_cast<int>(W), out.data_ptr<int64_t>(),
                    c10::hip::getCurrentHIPStream(oc.device().index()).stream());
    return out;
  }, py::arg("offsets"), py::arg("data"), py::arg("words"),
        "string keys -> [words + 1, n] int64: big-endian 8-byte words (sign-flipped) + byte length; signed order "
        "of the columns = lexicographic order of the strings");
  m.def("string_key_hash", [](const at::Tensor& offsets, const at::Tensor& data) {
    TFA_CHECK(offsets.scalar_type() == at::kLong && offsets.dim() == 1 && offsets.size(0) >= 1,
              "string_key_hash: offsets must be int64[n+1]");
    TFA_CHECK(data.scalar_type() == at::kByte && data.dim() == 1, "string_key_hash: data must be uint8[bytes]");
    TFA_CHECK(offsets.device() == data.device(), "string_key_hash: offsets and data on different devices");
    const int64_t n = offsets.size(0) - 1;
    at::Tensor oc = offsets.contiguous(), dc = data.contiguous();
    if (!oc.is_cuda()) {
      at::Tensor out = at::empty({2, n}, oc.options());
      const int64_t* o = oc.data_ptr<int64_t>();
      const uint8_t* d = dc.data_ptr<uint8_t>();
      int64_t* y = out.data_ptr<int64_t>();
      for (int64_t i = 0; i < n; ++i) {
        const int64_t a = o[i], len = o[i + 1] - a;
        uint64_t v = 0;
        for (int b = 0; b < 8; ++b) v |= static_cast<uint64_t>(b < len ? d[a + b] : 0) << (56 - 8 * b);
        y[i] = static_cast<int64_t>(v ^ 0x8000000000000000ull);
        y[n + i] = len > 8 ? static_cast<int64_t>(k::string_key_hash_host(d + a, len) + 9) : len;
      }
      return out;
    }
    c10::hip::HIPGuard guard(oc.device().index());
    at::Tensor out = pool_empty({2, n}, oc.options());
    k::string_key_hash(oc.data_ptr<int64_t>(), dc.data_ptr<uint8_t>(), n, out.data_ptr<int64_t>(),
                   c10::hip::getCurrentHIPStream(oc.device().index()).stream());
    return out;
  }, py::arg("offsets"), py::arg("data"),
        "bounded-width string keys -> [2, n] int64: sign-flipped big-endian word 0, tag = length for keys of "
        "<= 8 bytes, else 9 + a 62-bit hash of the whole key");
  m.def("string_verify", [](const at::Tensor& offsets, const at::Tensor& data, const at::Tensor& ids,
                            const at::Tensor& rep) {
    TFA_CHECK(offsets.scalar_type() == at::kLong && ids.scalar_type() == at::kLong && rep.scalar_type() == at::kLong,
              "string_verify: int64 offsets / ids / representatives");
    const int64_t n = offsets.size(0) - 1;
    TFA_CHECK(ids.dim() == 1 && ids.size(0) == n, "string_verify: one id per string");
    TFA_CHECK(offsets.device() == data.device() && ids.device() == data.device() && rep.device() == data.device(),
              "string_verify: tensors on different devices");
    at::Tensor oc = offsets.contiguous(), dc = data.contiguous(), ic = ids.contiguous(), rc = rep.contiguous();
    if (!oc.is_cuda()) {
      const int64_t* o = oc.data_ptr<int64_t>();
      const uint8_t* d = dc.data_ptr<uint8_t>();
      const int64_t* id = ic.data_ptr<int64_t>();
      const int64_t* r = rc.data_ptr<int64_t>();
      for (int64_t i = 0; i < n; ++i) {
        const int64_t a = o[i], len = o[i + 1] - a, q = r[id[i]];
        if (len <= 8 || q == i) continue;
        if (o[q + 1] - o[q] != len || std::memcmp(d + a, d + o[q], len) != 0) return false;
      }
      return true;
    }
    c10::hip::HIPGuard guard(oc.device().index());
    hipStream_t st = c10::hip::getCurrentHIPStream(oc.device().index()).stream();
    at::Tensor flag = pool_empty({1}, oc.options().dtype(at::kInt));
    TFA_CHECK(hipMemsetAsync(flag.data_ptr(), 0, sizeof(int), st) == hipSuccess, "string_verify: memset failed");
    k::string_verify(oc.data_ptr<int64_t>(), dc.data_ptr<uint8_t>(), ic.data_ptr<int64_t>(), rc.data_ptr<int64_t>(), n,
                     flag.data_ptr<int>(), st);
    return flag.item<int>() == 0;
  }, "True when every string equals its group representative's (no hash collision)");
  m.def("gather_strings", [](const at::Tensor& offsets, const at::Tensor& data, const at::Tensor& idx) {
    // rows idx of a device string column -> (host offsets [n+1], device bytes)
    TFA_CHECK(offsets.is_cuda() && data.is_cuda() && idx.is_cuda() && offsets.scalar_type() == at::kLong &&
                  idx.scalar_type() == at::kLong && data.scalar_type() == at::kByte,
              "gather_strings: device int64 offsets / idx and uint8 data expected");
    c10::hip::HIPGuard guard(data.device().index());
    hipStream_t st = c10::hip::getCurrentHIPStream(data.device().index()).stream();
    at::Tensor oc = offsets.contiguous(), ic = idx.contiguous(), dc = data.contiguous();
    const int64_t n = ic.numel();
    at::Tensor lens = pool_empty({std::max<int64_t>(n, 1)}, oc.options());
    k::string_lens(oc.data_ptr<int64_t>(), ic.data_ptr<int64_t>(), n, lens.data_ptr<int64_t>(), st);
    at::Tensor new_offs = at::empty({n + 1}, at::TensorOptions().dtype(at::kLong));
    int64_t* no = new_offs.data_ptr<int64_t>();
    no[0] = 0;
    if (n) {
      std::vector<int64_t> lh(n);
      TFA_CHECK(hipMemcpyAsync(lh.data(), lens.data_ptr(), n * sizeof(int64_t), hipMemcpyDeviceToHost, st) == hipSuccess &&
                    hipStreamSynchronize(st) == hipSuccess, "gather_strings: length copy failed");
      for (int64_t g = 0; g < n; ++g) no[g + 1] = no[g] + lh[g];
    }
    at::Tensor out = pool_empty({std::max<int64_t>(no[n], 1)}, dc.options());
    if (n) {
      at::Tensor dno = pool_empty({n + 1}, oc.options());
      TFA_CHECK(hipMemcpyAsync(dno.data_ptr(), no, (n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st) == hipSuccess,
                "gather_strings: offset copy failed");
      k::gather_bytes(dc.data_ptr<uint8_t>(), oc.data_ptr<int64_t>(), ic.data_ptr<int64_t>(), dno.data_ptr<int64_t>(), n,
                      out.data_ptr<uint8_t>(), st);
      TFA_CHECK(hipStreamSynchronize(st) == hipSuccess, "gather_strings: gather failed");  // `no` is pageable
    }
    return py::make_tuple(new_offs, out.narrow(0, 0, no[n]));
  }, "rows idx of a device string column -> (host int64 offsets [n+1], device uint8 bytes)");
  m.def("key_dest", [](const std::vector<at::Tensor>& keys, int64_t world) {
    TFA_CHECK(!keys.empty() && keys[0].is_cuda(), "key_dest: device key columns expected");
    c10::hip::HIPGuard guard(keys[0].device().index());
    const int64_t n = keys[0].size(0);
    hipStream_t s = c10::hip::getCurrentHIPStream(keys[0].device().index()).stream();
    at::Tensor h = pool_empty({n}, keys[0].options().dtype(at::kLong));
    for (size_t i = 0; i < keys.size(); ++i) {
      at::Tensor kc = keys[i].contiguous();
      TFA_CHECK(kc.dim() == 1 && kc.size(0) == n, "key_dest: key columns must be 1-D of equal length");
      k::key_hash(from_scalar_type(kc.scalar_type()), kc.data_ptr(), n,
                  reinterpret_cast<uint64_t*>(h.data_ptr<int64_t>()), i > 0, s);
    }
    at::Tensor dest = pool_empty({n}, h.options());
    k::hash_mod(reinterpret_cast<const uint64_t*>(h.data_ptr<int64_t>()), n, world, dest.data_ptr<int64_t>(), s);
    return dest;
  }, "destination rank of every row: hash(keys) % world (same on every rank)");
  m.def("group_representatives", [](const at::Tensor& ids, int64_t nseg) {
    TFA_CHECK(ids.is_cuda() && ids.scalar_type() == at::kLong && ids.dim() == 1, "group_representatives: device int64 ids");
    c10::hip::HIPGuard guard(ids.device().index());
    at::Tensor rep = pool_empty({nseg}, ids.options());
    k::group_representatives(ids.contiguous().data_ptr<int64_t>(), ids.size(0), nseg, rep.data_ptr<int64_t>(),
                             c10::hip::getCurrentHIPStream(ids.device().index()).stream());
    return rep;
  }, "the last row index of every group (device), as the host path's rep[ids] = arange(n)");
  m.def("partition_rows", [](const at::Tensor& dest0, int64_t world) {
    TFA_CHECK(dest0.is_cuda() && dest0.scalar_type() == at::kLong && dest0.dim() == 1, "partition_rows: device int64 dest");
    c10::hip::HIPGuard guard(dest0.device().index());
    at::Tensor dest = dest0.contiguous();
    const int64_t n = dest.size(0);
    hipStream_t s = c10::hip::getCurrentHIPStream(dest.device().index()).stream();
    const size_t wsb = k::partition_workspace_bytes(n);
    at::Tensor ws = pool_empty({static_cast<int64_t>(wsb)}, dest.options().dtype(at::kByte));
    at::Tensor perm = pool_empty({n}, dest.options());
    at::Tensor counts = pool_empty({world}, dest.options());
    k::partition_rows(dest.data_ptr<int64_t>(), n, world, perm.data_ptr<int64_t>(), counts.data_ptr<int64_t>(),
                      ws.data_ptr(), wsb, s);
    return py::make_tuple(perm, counts);
  }, "rows ordered by destination rank (stable) + rows per destination (device)");
  m.def("segment_csr", [](const at::Tensor& ids0, int64_t nseg) {
    TFA_CHECK(ids0.is_cuda() && ids0.dim() == 1 && (ids0.scalar_type() == at::kLong || ids0.scalar_type() == at::kInt),
              "segment_csr: device int ids");
    c10::hip::HIPGuard guard(ids0.device().index());
    at::Tensor ids = ids0.contiguous();
    const int64_t n = ids.size(0);
    hipStream_t s = c10::hip::getCurrentHIPStream(ids.device().index()).stream();
    at::Tensor perm = pool_empty({n}, ids.options().dtype(at::kLong));
    at::Tensor off = pool_empty({nseg + 1}, ids.options().dtype(at::kLong));
    const size_t wsb = k::segment_csr_workspace_bytes(n, nseg);
    at::Tensor ws = pool_empty({static_cast<int64_t>(wsb)}, ids.options().dtype(at::kByte));
    k::segment_csr(from_scalar_type(ids.scalar_type()), ids.data_ptr(), n, nseg, perm.data_ptr<int64_t>(),
                   off.data_ptr<int64_t>(), ws.data_ptr(), wsb, s);
    return py::make_tuple(perm, off);
  }, "ids [n] in [0, nseg) -> (rows ordered by segment, stable; CSR offsets [nseg + 1]) on the device");
  m.def("segment_rows", [](const at::Tensor& perm, const at::Tensor& offs, int64_t size) {
    TFA_CHECK(perm.is_cuda() && offs.is_cuda() && perm.scalar_type() == at::kLong && offs.scalar_type() == at::kLong,
              "segment_rows: device int64 tensors");
    c10::hip::HIPGuard guard(perm.device().index());
    const int64_t G = offs.size(0);
    at::Tensor idx = pool_empty({G * size}, perm.options());
    k::segment_rows(perm.contiguous().data_ptr<int64_t>(), offs.contiguous().data_ptr<int64_t>(), G, size,
                    idx.data_ptr<int64_t>(), c10::hip::getCurrentHIPStream(perm.device().index()).stream());
    return idx;
  }, "row ids of G equal-size segments: perm[offs[g] + j] for j < size -> [G * size]");
  m.def("scatter_rows", [](at::Tensor dst, const at::Tensor& idx, const at::Tensor& src0) {
    TFA_CHECK(dst.is_cuda() && idx.is_cuda() && src0.is_cuda() && idx.scalar_type() == at::kLong,
              "scatter_rows: device tensors");
    TFA_CHECK(dst.is_contiguous() && dst.dim() >= 1 && src0.scalar_type() == dst.scalar_type(),
              "scatter_rows: contiguous dst of the source dtype");
    c10::hip::HIPGuard guard(dst.device().index());
    at::Tensor src = src0.contiguous();
    TFA_CHECK(src.size(0) == idx.size(0), "scatter_rows: one index per source row");
    const int64_t row = dst.size(0) ? dst.numel() / dst.size(0) : 0;
    TFA_CHECK(src.numel() == idx.size(0) * row, "scatter_rows: source rows must match the destination row shape");
    k::scatter_rows(row * dst.element_size(), src.data_ptr(), idx.contiguous().data_ptr<int64_t>(), dst.data_ptr(),
                    idx.size(0), c10::hip::getCurrentHIPStream(dst.device().index()).stream());
    return dst;
  }, "dst[idx[j]] = src[j] along dim 0 (device scatter kernel), in place");
  // one record per row holding every column (the keyed shuffle's single
  // all-to-all payload): column c at byte offset offs[c] of R-byte records
  m.def("pack_rows", [](const std::vector<at::Tensor>& cols, std::optional<at::Tensor> perm) {
    TFA_CHECK(!cols.empty() && cols.size() <= static_cast<size_t>(k::kMaxPackCols), "pack_rows: 1..16 columns");
    const int64_t n = perm ? perm->size(0) : cols[0].size(0);
    k::PackCols pc;
    pc.n = static_cast<int>(cols.size());
    std::vector<at::Tensor> keep;
    int64_t R = 0;
    for (size_t c = 0; c < cols.size(); ++c) {
      at::Tensor t = cols[c].contiguous();
      TFA_CHECK(t.is_cuda() && t.dim() >= 1 && t.device() == cols[0].device(), "pack_rows: device columns");
      TFA_CHECK(perm || t.size(0) == n, "pack_rows: columns disagree on rows");
      const int64_t rb = t.size(0) ? t.numel() / t.size(0) * t.element_size() : 0;
      pc.row_bytes[c] = rb;
      pc.off[c] = R;
      pc.ptr[c] = t.data_ptr();
      R += (rb + 3) / 4 * 4;
      keep.push_back(t);
    }
    c10::hip::HIPGuard guard(cols[0].device().index());
    at::Tensor out = pool_empty({n, R}, cols[0].options().dtype(at::kByte));
    const int64_t* pp = nullptr;
    at::Tensor pc_t;
    if (perm) {
      pc_t = perm->contiguous();
      TFA_CHECK(pc_t.is_cuda() && pc_t.scalar_type() == at::kLong, "pack_rows: device int64 perm");
      pp = pc_t.data_ptr<int64_t>();
    }
    k::pack_rows(pc, pp, n, R, out.data_ptr(), c10::hip::getCurrentHIPStream(cols[0].device().index()).stream());
    std::vector<int64_t> offs(pc.off, pc.off + pc.n);
    return py::make_tuple(out, offs);
  }, py::arg("cols"), py::arg("perm") = py::none(),
     "device columns -> (uint8 records [n, R] in perm order, byte offset of each column)");
  m.def("unpack_rows", [](const at::Tensor& rec, const std::vector<at::Tensor>& outs) {
    TFA_CHECK(rec.is_cuda() && rec.dim() == 2 && rec.scalar_type() == at::kByte, "unpack_rows: device uint8 records");
    TFA_CHECK(!outs.empty() && outs.size() <= static_cast<size_t>(k::kMaxPackCols), "unpack_rows: 1..16 columns");
    const int64_t n = rec.size(0);
    k::PackCols pc;
    pc.n = static_cast<int>(outs.size());
    int64_t R = 0;
    for (size_t c = 0; c < outs.size(); ++c) {
      const at::Tensor& t = outs[c];
      TFA_CHECK(t.is_cuda() && t.is_contiguous() && t.size(0) == n, "unpack_rows: contiguous device outputs of n rows");
      const int64_t rb = n ? t.numel() / n * t.element_size() : 0;
      pc.row_bytes[c] = rb;
      pc.off[c] = R;
      pc.ptr[c] = t.data_ptr();
      R += (rb + 3) / 4 * 4;
    }
    TFA_CHECK(R == rec.size(1), "unpack_rows: record width ", rec.size(1), " does not match the columns (", R, ")");
    c10::hip::HIPGuard guard(rec.device().index());
    k::unpack_rows(pc, rec.contiguous().data_ptr(), n, R, c10::hip::getCurrentHIPStream(rec.device().index()).stream());
  }, "records [n, R] -> the preallocated device columns (same layout as pack_rows)");
  // DataFrame.filter on device-resident partitions (kernels/compact.hip)
  m.def("compact_tile_rows", [] { return k::compact_tile_rows(); }, "rows per tile of the row-compaction kernels");
  m.def("compact_rows", [](const at::Tensor& mask0, const std::vector<at::Tensor>& cols, bool want_index) {
    if (cols.empty() || cols.size() > static_cast<size_t>(k::kMaxPackCols))
      throw py::value_error(str_cat("compact_rows: 1..", k::kMaxPackCols, " columns per call, got ", cols.size()));
    if (mask0.scalar_type() != at::kBool && mask0.scalar_type() != at::kByte)
      throw py::type_error(str_cat("compact_rows: the mask must be bool or uint8, got ", c10::toString(mask0.scalar_type())));
    if (!mask0.is_cuda()) throw py::value_error("compact_rows: the mask must be a device tensor");
    if (cols[0].dim() < 1) throw py::value_error("compact_rows: columns need a row dimension");
    const int64_t n = cols[0].size(0);
    if (mask0.dim() != 1 || mask0.size(0) != n)
      throw py::value_error(str_cat("compact_rows: the mask must hold one entry per row ([", n, "]), got ",
                                    mask0.dim(), "-D with ", mask0.numel(), " entries"));
    std::vector<at::Tensor> src;
    for (size_t c = 0; c < cols.size(); ++c) {
      const at::Tensor& t = cols[c];
      if (!t.is_cuda() || t.device() != mask0.device())
        throw py::value_error(str_cat("compact_rows: column ", c, " is not on the mask's device"));
      if (t.dim() < 1 || t.size(0) != n)
        throw py::value_error(str_cat("compact_rows: column ", c, " has ", t.dim() < 1 ? 0 : t.size(0),
                                      " rows, column 0 has ", n));
      src.push_back(t.contiguous());
    }
    c10::hip::HIPGuard guard(mask0.device().index());
    hipStream_t s = c10::hip::getCurrentHIPStream(mask0.device().index()).stream();
    at::Tensor mask = mask0.contiguous();
    const uint8_t* mp = static_cast<const uint8_t*>(mask.data_ptr());
    int64_t total = 0;
    at::Tensor ws;
    if (n > 0) {
      const size_t wsb = k::compact_workspace_bytes(n);
      // (int64 elements: the workspace starts with 64-bit offsets)
      ws = pool_empty({static_cast<int64_t>((wsb + 7) / 8)}, mask.options().dtype(at::kLong));
      py::gil_scoped_release nogil;
      total = k::compact_plan(mp, n, ws.data_ptr(), ws.numel() * 8, s);
    }
    k::PackCols ps, pd;
    ps.n = pd.n = static_cast<int>(src.size());
    std::vector<at::Tensor> outs;
    for (size_t c = 0; c < src.size(); ++c) {
      std::vector<int64_t> shape = src[c].sizes().vec();
      int64_t cell = 1;
      for (size_t d = 1; d < shape.size(); ++d) cell *= shape[d];
      shape[0] = total;
      at::Tensor o = pool_empty(shape, src[c].options());
      ps.row_bytes[c] = pd.row_bytes[c] = cell * static_cast<int64_t>(src[c].element_size());
      ps.off[c] = pd.off[c] = 0;
      ps.ptr[c] = src[c].data_ptr();
      pd.ptr[c] = o.data_ptr();
      outs.push_back(o);
    }
    py::object index = py::none();
    int64_t* ip = nullptr;
    if (want_index) {
      at::Tensor it = pool_empty({total}, mask.options().dtype(at::kLong));
      ip = it.data_ptr<int64_t>();
      index = py::cast(it);
    }
    if (n > 0 && total > 0) k::compact_gather(ps, pd, mp, n, total, ws.data_ptr(), ip, s);
    return py::make_tuple(outs, total, index);
  }, py::arg("mask"), py::arg("cols"), py::arg("want_index") = false,
     "rows of the device columns whose mask entry is non-zero, in order -> (compacted columns, kept count, "
     "int64 indices of the kept rows or None); one stream synchronisation reads the count");
  // DataFrame.orderBy / sortWithinPartitions on device-resident partitions (kernels/sort.hip)
  m.def("sort_tile_rows", [] { return k::sort_tile_rows(); }, "keys per block of the radix sort under sort_argsort");
  m.def("sort_encode", [](const std::vector<at::Tensor>& keys, const std::vector<bool>& descending) {
    if (keys.empty() || keys.size() > static_cast<size_t>(k::kMaxSortKeys))
      throw py::value_error(str_cat("sort_encode: 1..", k::kMaxSortKeys, " keys per call, got ", keys.size()));
    if (descending.size() != keys.size())
      throw py::value_error(str_cat("sort_encode: ", descending.size(), " directions for ", keys.size(), " keys"));
    if (!keys[0].is_cuda()) throw py::value_error("sort_encode: the keys must be device tensors");
    if (keys[0].dim() != 1) throw py::value_error("sort_encode: keys must be 1-D (one scalar per row)");
    const int64_t n = keys[0].size(0);
    k::SortKeys sk;
    sk.n = static_cast<int>(keys.size());
    std::vector<at::Tensor> keep;
    for (size_t c = 0; c < keys.size(); ++c) {
      const at::Tensor& t = keys[c];
      if (!t.is_cuda() || t.device() != keys[0].device())
        throw py::value_error(str_cat("sort_encode: key ", c, " is not on the first key's device"));
      if (t.dim() != 1 || t.size(0) != n)
        throw py::value_error(str_cat("sort_encode: key ", c, " must be 1-D with ", n, " rows"));
      const auto st = t.scalar_type();
      if (st != at::kFloat && st != at::kDouble && st != at::kLong && st != at::kInt && st != at::kShort &&
          st != at::kChar && st != at::kByte && st != at::kBool)
        throw py::type_error(str_cat("sort_encode: ", c10::toString(st), " is not supported as a sort key"));
      keep.push_back(t.contiguous());
      sk.dtype[c] = from_scalar_type(st);
      sk.ptr[c] = keep.back().data_ptr();
      sk.descending[c] = descending[c] ? 1 : 0;
    }
    c10::hip::HIPGuard guard(keys[0].device().index());
    at::Tensor words = pool_empty({static_cast<int64_t>(keys.size()), n}, keys[0].options().dtype(at::kLong));
    k::sort_encode(sk, n, words.data_ptr<int64_t>(), c10::hip::getCurrentHIPStream(keys[0].device().index()).stream());
    return words;
  }, py::arg("keys"), py::arg("descending"),
     "device key columns [n] + a descending flag each -> int64 [keys, n]: one order-preserving unsigned word per "
     "key and row (bit patterns)");
  m.def("sort_argsort", [](const at::Tensor& words0) {
    if (!words0.is_cuda() || words0.scalar_type() != at::kLong || words0.dim() != 2)
      throw py::value_error("sort_argsort: device int64 words [W, n] expected");
    if (words0.size(0) < 1 || words0.size(0) > k::kMaxSortKeys)
      throw py::value_error(str_cat("sort_argsort: 1..", k::kMaxSortKeys, " words per row, got ", words0.size(0)));
    c10::hip::HIPGuard guard(words0.device().index());
    hipStream_t s = c10::hip::getCurrentHIPStream(words0.device().index()).stream();
    at::Tensor words = words0.contiguous();
    const int W = static_cast<int>(words.size(0));
    const int64_t n = words.size(1);
    at::Tensor perm = pool_empty({n}, words.options());
    g_sort_last_passes = 0;
    if (n > 0) {
      const size_t wsb = k::sort_argsort_workspace_bytes(W, n);
      at::Tensor ws = pool_empty({static_cast<int64_t>((wsb + 7) / 8)}, words.options());
      py::gil_scoped_release nogil;
      g_sort_last_passes = k::sort_argsort(words.data_ptr<int64_t>(), W, n, perm.data_ptr<int64_t>(), ws.data_ptr(),
                                           static_cast<size_t>(ws.numel()) * 8, s);
    }
    return perm;
  }, py::arg("words"),
     "words [W, n] (sort_encode) -> int64 perm [n]: perm[j] = source row of output row j, stable; only the 8-bit "
     "digits that vary are sorted (one stream synchronisation reads the masks)");
  m.def("sort_last_passes", [] { return g_sort_last_passes; },
        "radix passes of the calling thread's last sort_argsort");
  m.def("permute_rows", [](const at::Tensor& perm0, const std::vector<at::Tensor>& cols) {
    if (cols.empty() || cols.size() > static_cast<size_t>(k::kMaxPackCols))
      throw py::value_error(str_cat("permute_rows: 1..", k::kMaxPackCols, " columns per call, got ", cols.size()));
    if (perm0.scalar_type() != at::kLong)
      throw py::type_error(str_cat("permute_rows: the permutation must be int64, got ", c10::toString(perm0.scalar_type())));
    if (!perm0.is_cuda()) throw py::value_error("permute_rows: the permutation must be a device tensor");
    if (cols[0].dim() < 1) throw py::value_error("permute_rows: columns need a row dimension");
    const int64_t n = cols[0].size(0);
    if (perm0.dim() != 1 || perm0.size(0) != n)
      throw py::value_error(str_cat("permute_rows: the permutation must hold one entry per row ([", n, "]), got ",
                                    perm0.dim(), "-D with ", perm0.numel(), " entries"));
    std::vector<at::Tensor> src;
    for (size_t c = 0; c < cols.size(); ++c) {
      const at::Tensor& t = cols[c];
      if (!t.is_cuda() || t.device() != perm0.device())
        throw py::value_error(str_cat("permute_rows: column ", c, " is not on the permutation's device"));
      if (t.dim() < 1 || t.size(0) != n)
        throw py::value_error(str_cat("permute_rows: column ", c, " has ", t.dim() < 1 ? 0 : t.size(0),
                                      " rows, column 0 has ", n));
      src.push_back(t.contiguous());
    }
    c10::hip::HIPGuard guard(perm0.device().index());
    hipStream_t s = c10::hip::getCurrentHIPStream(perm0.device().index()).stream();
    at::Tensor perm = perm0.contiguous();
    k::PackCols ps, pd;
    ps.n = pd.n = static_cast<int>(src.size());
    std::vector<at::Tensor> outs;
    for (size_t c = 0; c < src.size(); ++c) {
      at::Tensor o = pool_empty(src[c].sizes().vec(), src[c].options());
      const int64_t rb = n ? src[c].numel() / n * static_cast<int64_t>(src[c].element_size()) : 0;
      ps.row_bytes[c] = pd.row_bytes[c] = rb;
      ps.off[c] = pd.off[c] = 0;
      ps.ptr[c] = src[c].data_ptr();
      pd.ptr[c] = o.data_ptr();
      outs.push_back(o);
    }
    if (n > 0) k::permute_rows(ps, pd, perm.data_ptr<int64_t>(), n, s);
    return outs;
  }, py::arg("perm"), py::arg("cols"),
     "output row j of every device column = its row perm[j] (perm: a device int64 permutation of the rows), all "
     "columns in one launch");
  m.def("sort_bounds", [](const at::Tensor& words0, const at::Tensor& perm0, const at::Tensor& splitters0) {
    if (!words0.is_cuda() || words0.scalar_type() != at::kLong || words0.dim() != 2)
      throw py::value_error("sort_bounds: device int64 words [W, n] expected");
    const int64_t W = words0.size(0), n = words0.size(1);
    if (W < 1 || W > k::kMaxSortKeys)
      throw py::value_error(str_cat("sort_bounds: 1..", k::kMaxSortKeys, " words per row, got ", W));
    if (!perm0.is_cuda() || perm0.device() != words0.device() || perm0.scalar_type() != at::kLong ||
        perm0.dim() != 1 || perm0.size(0) != n)
      throw py::value_error(str_cat("sort_bounds: a device int64 permutation [", n, "] on the words' device expected"));
    if (splitters0.scalar_type() != at::kLong || splitters0.dim() != 2 || splitters0.size(1) != W)
      throw py::value_error(str_cat("sort_bounds: int64 splitters [S, ", W, "] expected"));
    c10::hip::HIPGuard guard(words0.device().index());
    hipStream_t s = c10::hip::getCurrentHIPStream(words0.device().index()).stream();
    at::Tensor words = words0.contiguous(), perm = perm0.contiguous();
    at::Tensor sp = splitters0.to(words0.device()).contiguous();
    const int64_t S = sp.size(0);
    at::Tensor out = pool_empty({S}, words.options());
    k::sort_bounds(words.data_ptr<int64_t>(), static_cast<int>(W), n, perm.data_ptr<int64_t>(), sp.data_ptr<int64_t>(),
                   S, out.data_ptr<int64_t>(), s);
    return out;
  }, py::arg("words"), py::arg("perm"), py::arg("splitters"),
     "for each splitter tuple [W]: the number of rows of the sorted order whose word tuple is lexicographically "
     "(unsigned) below it -> device int64 [S]");
  m.def("take_rows", [](const at::Tensor& idx0, const std::vector<at::Tensor>& cols) {
    if (cols.empty() || cols.size() > static_cast<size_t>(k::kMaxPackCols))
      throw py::value_error(str_cat("take_rows: 1..", k::kMaxPackCols, " columns per call, got ", cols.size()));
    if (idx0.scalar_type() != at::kLong)
      throw py::type_error(str_cat("take_rows: the row indices must be int64, got ", c10::toString(idx0.scalar_type())));
    if (!idx0.is_cuda()) throw py::value_error("take_rows: the row indices must be a device tensor");
    if (idx0.dim() != 1) throw py::value_error(str_cat("take_rows: the row indices must be 1-D, got ", idx0.dim(), "-D"));
    if (cols[0].dim() < 1) throw py::value_error("take_rows: columns need a row dimension");
    const int64_t n_src = cols[0].size(0), n_out = idx0.size(0);
    if (n_out > 0 && n_src == 0) throw py::value_error("take_rows: rows asked of columns without rows");
    std::vector<at::Tensor> src;
    for (size_t c = 0; c < cols.size(); ++c) {
      const at::Tensor& t = cols[c];
      if (!t.is_cuda() || t.device() != idx0.device())
        throw py::value_error(str_cat("take_rows: column ", c, " is not on the indices' device"));
      if (t.dim() < 1 || t.size(0) != n_src)
        throw py::value_error(str_cat("take_rows: column ", c, " has ", t.dim() < 1 ? 0 : t.size(0),
                                      " rows, column 0 has ", n_src));
      src.push_back(t.contiguous());
    }
    c10::hip::HIPGuard guard(idx0.device().index());
    hipStream_t s = c10::hip::getCurrentHIPStream(idx0.device().index()).stream();
    at::Tensor idx = idx0.contiguous();
    k::PackCols ps, pd;
    ps.n = pd.n = static_cast<int>(src.size());
    std::vector<at::Tensor> outs;
    for (size_t c = 0; c < src.size(); ++c) {
      std::vector<int64_t> shape = src[c].sizes().vec();
      int64_t cell = 1;
      for (size_t d = 1; d < shape.size(); ++d) cell *= shape[d];
      shape[0] = n_out;
      at::Tensor o = pool_empty(shape, src[c].options());
      ps.row_bytes[c] = pd.row_bytes[c] = cell * static_cast<int64_t>(src[c].element_size());
      ps.off[c] = pd.off[c] = 0;
      ps.ptr[c] = src[c].data_ptr();
      pd.ptr[c] = o.data_ptr();
      outs.push_back(o);
    }
    if (n_out > 0) k::take_rows(ps, pd, idx.data_ptr<int64_t>(), n_out, n_src, s);
    return outs;
  }, py::arg("idx"), py::arg("cols"),
     "output row j of every device column = its row idx[j] (idx: device int64 [n_out], entries in [0, rows), "
     "repeats allowed), all columns in one launch");
  // DataFrame.dropDuplicates / distinct on device-resident partitions (kernels/unique.hip)
  m.def("unique_tile_rows", [] { return k::unique_tile_rows(); }, "positions per tile of unique_rows");
  m.def("unique_rows", [](const at::Tensor& words0, std::optional<at::Tensor> perm0) {
    if (!words0.is_cuda()) throw py::value_error("unique_rows: the words must be a device tensor");
    if (words0.scalar_type() != at::kLong)
      throw py::type_error(str_cat("unique_rows: the words must be int64, got ", c10::toString(words0.scalar_type())));
    if (words0.dim() != 2) throw py::value_error(str_cat("unique_rows: words [W, n] expected, got ", words0.dim(), "-D"));
    const int64_t W = words0.size(0), n = words0.size(1);
    if (W < 1 || W > k::kMaxSortKeys)
      throw py::value_error(str_cat("unique_rows: 1..", k::kMaxSortKeys, " words per row, got ", W));
    if (!words0.is_contiguous()) throw py::value_error("unique_rows: the words must be contiguous");
    const int64_t* pp = nullptr;
    at::Tensor perm;
    if (perm0.has_value()) {
      if (perm0->scalar_type() != at::kLong)
        throw py::type_error(str_cat("unique_rows: the order must be int64, got ", c10::toString(perm0->scalar_type())));
      if (!perm0->is_cuda() || perm0->device() != words0.device())
        throw py::value_error("unique_rows: the order must be a device tensor on the words' device");
      if (perm0->dim() != 1 || perm0->size(0) != n)
        throw py::value_error(str_cat("unique_rows: the order must hold one entry per row ([", n, "]), got ",
                                      perm0->dim(), "-D with ", perm0->numel(), " entries"));
      perm = perm0->contiguous();
      pp = perm.data_ptr<int64_t>();
    }
    c10::hip::HIPGuard guard(words0.device().index());
    hipStream_t s = c10::hip::getCurrentHIPStream(words0.device().index()).stream();
    if (n == 0) return pool_empty({0}, words0.options());
    const size_t wsb = k::unique_workspace_bytes(n);
    // (int64 elements: the workspace starts with 64-bit offsets)
    at::Tensor ws = pool_empty({static_cast<int64_t>((wsb + 7) / 8)}, words0.options());
    int64_t total = 0;
    {
      py::gil_scoped_release nogil;
      total = k::unique_plan(words0.data_ptr<int64_t>(), static_cast<int>(W), n, pp, ws.data_ptr(), ws.numel() * 8, s);
    }
    at::Tensor kept = pool_empty({total}, words0.options());
    k::unique_write(pp, n, total, ws.data_ptr(), kept.data_ptr<int64_t>(), s);
    return kept;
  }, py::arg("words"), py::arg("perm") = py::none(),
     "words [W, n] (sort_encode) in the stable order perm (sort_argsort; None: in order already) -> int64 [m]: "
     "perm[i] of every position i that starts a run of equal word tuples, in order (source row indices for "
     "take_rows); one stream synchronisation reads the count");
  // groupBy().pivot().agg on device-resident partitions (kernels/pivot.hip)
  m.def("pivot_block_threads", [] { return k::pivot_block_threads(); }, "threads per block of pivot_spread");
  m.def("pivot_spread", [](const at::Tensor& offsets, const at::Tensor& pivot_words, const at::Tensor& value_words,
                           const std::vector<at::Tensor>& vals, const std::vector<int64_t>& fills) {
    auto words1d = [&](const at::Tensor& t, const char* name) {
      if (!t.is_cuda()) throw py::value_error(str_cat("pivot_spread: ", name, " must be a device tensor"));
      if (t.scalar_type() != at::kLong)
        throw py::type_error(str_cat("pivot_spread: ", name, " must be int64, got ", c10::toString(t.scalar_type())));
      if (t.device() != offsets.device())
        throw py::value_error(str_cat("pivot_spread: ", name, " is not on the offsets' device"));
      if (t.dim() != 1 || !t.is_contiguous())
        throw py::value_error(str_cat("pivot_spread: ", name, " must be 1-D and contiguous"));
    };
    words1d(offsets, "offsets");
    words1d(pivot_words, "pivot_words");
    words1d(value_words, "value_words");
    if (offsets.size(0) < 1)
      throw py::value_error("pivot_spread: offsets [G + 1] expected, got an empty tensor");
    const int64_t G = offsets.size(0) - 1, mm = pivot_words.size(0), V = value_words.size(0);
    if (V > k::kMaxPivotValues)
      throw py::value_error(str_cat("pivot_spread: at most ", k::kMaxPivotValues, " values per call, got ", V));
    if (vals.empty() || vals.size() > static_cast<size_t>(k::kMaxPackCols))
      throw py::value_error(str_cat("pivot_spread: 1..", k::kMaxPackCols, " outputs per call, got ", vals.size()));
    if (fills.size() != vals.size())
      throw py::value_error(str_cat("pivot_spread: ", fills.size(), " fills for ", vals.size(), " outputs"));
    k::PivotSpreadCols pc;
    pc.n = static_cast<int>(vals.size());
    c10::hip::HIPGuard guard(offsets.device().index());
    std::vector<at::Tensor> outs;
    for (size_t a = 0; a < vals.size(); ++a) {
      const at::Tensor& v = vals[a];
      if (!v.is_cuda() || v.device() != offsets.device())
        throw py::value_error(str_cat("pivot_spread: vals[", a, "] must be a device tensor on the offsets' device"));
      if (v.element_size() != 4 && v.element_size() != 8)
        throw py::type_error(str_cat("pivot_spread: vals[", a, "] has ", c10::toString(v.scalar_type()),
                                     " elements; 4- or 8-byte elements expected"));
      if (v.dim() != 1 || v.size(0) != mm || !v.is_contiguous())
        throw py::value_error(str_cat("pivot_spread: vals[", a, "] must be contiguous [", mm,
                                      "], one element per pivot word"));
      outs.push_back(pool_empty({V, G}, v.options()));
      if (v.element_size() == 8) pc.wide |= 1u << a;
      pc.src[a] = v.data_ptr();
      pc.dst[a] = outs.back().data_ptr();
      pc.fill[a] = fills[a];
    }
    if (G > 0 && V > 0)
      k::pivot_spread(offsets.data_ptr<int64_t>(), mm ? pivot_words.data_ptr<int64_t>() : nullptr,
                      value_words.data_ptr<int64_t>(), G, mm, V, pc,
                      c10::hip::getCurrentHIPStream(offsets.device().index()).stream());
    return outs;
  }, py::arg("offsets"), py::arg("pivot_words"), py::arg("value_words"), py::arg("vals"), py::arg("fills"),
     "offsets int64 [G + 1] (CSR of the keys over the records), pivot_words int64 [m] (ascending as unsigned words "
     "inside every key, each at most once), value_words int64 [V <= 1024], vals: 1..16 contiguous device columns [m] "
     "of 4- or 8-byte elements, fills: one int64 bit pattern per column -> one tensor [V, G] per column: cell [j, g] "
     "is vals[a] at the record of key g whose word is value_words[j], else the fill (its low 4 bytes for 4-byte "
     "elements). Bit copies; every cell is written once, no atomics");
  // DataFrame.join on device-resident partitions (kernels/join.hip)
  m.def("join_tile_rows", [] { return k::join_tile_rows(); }, "output rows per block of join_expand");
  m.def("join_gather_words", [](const at::Tensor& words0, const at::Tensor& perm0) {
    if (!words0.is_cuda() || words0.scalar_type() != at::kLong || words0.dim() != 2)
      throw py::value_error("join_gather_words: device int64 words [W, m] expected");
    const int64_t W = words0.size(0), mm = words0.size(1);
    if (W < 1 || W > k::kMaxSortKeys)
      throw py::value_error(str_cat("join_gather_words: 1..", k::kMaxSortKeys, " words per row, got ", W));
    if (!perm0.is_cuda() || perm0.device() != words0.device() || perm0.scalar_type() != at::kLong ||
        perm0.dim() != 1 || perm0.size(0) != mm)
      throw py::value_error(str_cat("join_gather_words: a device int64 permutation [", mm,
                                    "] on the words' device expected"));
    c10::hip::HIPGuard guard(words0.device().index());
    hipStream_t s = c10::hip::getCurrentHIPStream(words0.device().index()).stream();
    at::Tensor words = words0.contiguous(), perm = perm0.contiguous();
    at::Tensor out = pool_empty({W, mm}, words.options());
    k::join_gather_words(words.data_ptr<int64_t>(), static_cast<int>(W), mm, perm.data_ptr<int64_t>(),
                         out.data_ptr<int64_t>(), s);
    return out;
  }, py::arg("words"), py::arg("perm"),
     "words [W, m] in the order perm (sort_argsort): out[w, j] = words[w, perm[j]]");
  m.def("join_probe", [](const at::Tensor& left0, const at::Tensor& right0, int mask_mode) {
    if (!left0.is_cuda() || left0.dim() != 2)
      throw py::value_error("join_probe: device int64 left words [W, n] expected");
    if (left0.scalar_type() != at::kLong || right0.scalar_type() != at::kLong)
      throw py::type_error(str_cat("join_probe: the words must be int64, got ", c10::toString(left0.scalar_type()),
                                   " and ", c10::toString(right0.scalar_type())));
    if (!right0.is_cuda() || right0.device() != left0.device() || right0.dim() != 2)
      throw py::value_error("join_probe: device int64 build words [W, m] on the left words' device expected");
    const int64_t W = left0.size(0), n = left0.size(1), mm = right0.size(1);
    if (W < 1 || W > k::kMaxSortKeys)
      throw py::value_error(str_cat("join_probe: 1..", k::kMaxSortKeys, " words per row, got ", W));
    if (right0.size(0) != W)
      throw py::value_error(str_cat("join_probe: ", W, " words per left row, ", right0.size(0), " per build row"));
    if (mask_mode < 0 || mask_mode > 2)
      throw py::value_error(str_cat("join_probe: mask 0 (none), 1 (matched) or 2 (unmatched) expected, got ", mask_mode));
    c10::hip::HIPGuard guard(left0.device().index());
    hipStream_t s = c10::hip::getCurrentHIPStream(left0.device().index()).stream();
    at::Tensor left = left0.contiguous(), right = right0.contiguous();
    at::Tensor lo = pool_empty({n}, left.options()), cnt = pool_empty({n}, left.options());
    py::object mask = py::none();
    uint8_t* mp = nullptr;
    if (mask_mode != 0) {
      at::Tensor mt = pool_empty({n}, left.options().dtype(at::kBool));
      mp = static_cast<uint8_t*>(mt.data_ptr());
      mask = py::cast(mt);
    }
    k::join_probe(left.data_ptr<int64_t>(), static_cast<int>(W), n, mm ? right.data_ptr<int64_t>() : nullptr, mm,
                  lo.data_ptr<int64_t>(), cnt.data_ptr<int64_t>(), mp, mask_mode, s);
    return py::make_tuple(lo, cnt, mask);
  }, py::arg("left"), py::arg("right_sorted"), py::arg("mask") = 0,
     "left words [W, n] against the build side's words in sorted order [W, m] -> (lo [n]: sorted positions below "
     "the row's tuple, cnt [n]: positions equal to it, bool mask [n] or None: cnt != 0 for mask=1, cnt == 0 for "
     "mask=2)");
  m.def("join_expand", [](const at::Tensor& lo0, const at::Tensor& cnt0, const at::Tensor& perm0) {
    if (lo0.scalar_type() != at::kLong || cnt0.scalar_type() != at::kLong || perm0.scalar_type() != at::kLong)
      throw py::type_error("join_expand: int64 lo, cnt and perm expected");
    if (!lo0.is_cuda() || !cnt0.is_cuda() || !perm0.is_cuda() || cnt0.device() != lo0.device() ||
        perm0.device() != lo0.device())
      throw py::value_error("join_expand: lo, cnt and perm must be tensors on one device");
    if (lo0.dim() != 1 || cnt0.dim() != 1 || perm0.dim() != 1 || cnt0.size(0) != lo0.size(0))
      throw py::value_error("join_expand: lo [n], cnt [n] and perm [m] expected");
    const int64_t n = lo0.size(0), mm = perm0.size(0);
    c10::hip::HIPGuard guard(lo0.device().index());
    hipStream_t s = c10::hip::getCurrentHIPStream(lo0.device().index()).stream();
    at::Tensor lo = lo0.contiguous(), cnt = cnt0.contiguous(), perm = perm0.contiguous();
    at::Tensor offs = pool_empty({n + 1}, lo.options());
    int64_t total = 0;
    {
      const size_t wsb = k::join_scan_workspace_bytes(n);
      at::Tensor ws = pool_empty({static_cast<int64_t>((wsb + 7) / 8)}, lo.options());
      py::gil_scoped_release nogil;
      total = k::join_scan(cnt.data_ptr<int64_t>(), n, mm, offs.data_ptr<int64_t>(), ws.data_ptr(),
                           static_cast<size_t>(ws.numel()) * 8, s);
    }
    at::Tensor li = pool_empty({total}, lo.options()), ri = pool_empty({total}, lo.options());
    k::join_expand(offs.data_ptr<int64_t>(), lo.data_ptr<int64_t>(), perm.data_ptr<int64_t>(), n, mm, total,
                   li.data_ptr<int64_t>(), ri.data_ptr<int64_t>(), s);
    return py::make_tuple(li, ri, offs);
  }, py::arg("lo"), py::arg("cnt"), py::arg("perm"),
     "join_probe's lo / cnt [n] and the build side's permutation [m] -> (left_idx [total], right_idx [total], offs "
     "[n + 1]): the exclusive scan of cnt, and per output row the left row and the matching build row, left rows in "
     "order, a row's matches in sorted (= build row) order; one stream synchronisation reads the total");
  // DataFrame.describe / summary / approxQuantile on device-resident columns (kernels/stats.hip)
  m.def("stats_tile_rows", [] { return k::stats_tile_rows(); }, "rows per tile of select_hist");
  m.def("column_moments", [](const std::vector<at::Tensor>& cols) {
    const k::StatCols sc = stat_cols_from("column_moments", cols);
    const int64_t n = cols[0].size(0), C = sc.n;
    const auto dev = cols[0].device();
    if (n == 0) {  // nothing is launched
      at::Tensor mo = at::empty({C, 3}, at::kDouble), ex = at::empty({C, 2}, at::kLong);
      for (int64_t c = 0; c < C; ++c) {
        mo.data_ptr<double>()[3 * c] = 0.0;
        mo.data_ptr<double>()[3 * c + 1] = mo.data_ptr<double>()[3 * c + 2] = std::numeric_limits<double>::quiet_NaN();
        ex.data_ptr<int64_t>()[2 * c] = -1;  // (all ones)
        ex.data_ptr<int64_t>()[2 * c + 1] = 0;
      }
      return py::make_tuple(mo.to(dev), ex.to(dev));
    }
    c10::hip::HIPGuard guard(dev.index());
    hipStream_t s = c10::hip::getCurrentHIPStream(dev.index()).stream();
    at::Tensor mo = pool_empty({C, 3}, cols[0].options().dtype(at::kDouble));
    at::Tensor ex = pool_empty({C, 2}, cols[0].options().dtype(at::kLong));
    const size_t wsb = k::column_moments_workspace_bytes(sc.n, n);
    at::Tensor ws = pool_empty({static_cast<int64_t>((wsb + 7) / 8)}, cols[0].options().dtype(at::kLong));
    k::column_moments(sc, n, mo.data_ptr<double>(), ex.data_ptr<int64_t>(), ws.data_ptr(),
                      static_cast<size_t>(ws.numel()) * 8, s);
    return py::make_tuple(mo, ex);
  }, py::arg("cols"),
     "up to 16 dense scalar device columns [n] (mixed dtypes, contiguous) -> (moments f64 [C, 3]: n, mean, M2 = the "
     "sum of squared deviations; extremes int64 [C, 2]: the smallest and largest order-preserving word, bit "
     "patterns), device tensors; the same bits on every run. n == 0 gives (0, NaN, NaN) and (all ones, 0)");
  m.def("select_hist", [](const at::Tensor& col, const at::Tensor& prefixes0, int prefix_bits) {
    stat_column("select_hist", col, "the column");
    if (prefixes0.scalar_type() != at::kLong || prefixes0.dim() != 1)
      throw py::value_error("select_hist: int64 prefixes [P] expected");
    const int64_t P = prefixes0.size(0);
    if (P < 1 || P > k::kMaxPackCols)
      throw py::value_error(str_cat("select_hist: 1..", k::kMaxPackCols, " prefixes per call, got ", P));
    if (prefix_bits < 0 || prefix_bits > 56 || prefix_bits % 8 != 0)
      throw py::value_error(str_cat("select_hist: prefix_bits must be one of 0, 8, ..., 56, got ", prefix_bits));
    if (prefix_bits == 0 && P != 1)
      throw py::value_error(str_cat("select_hist: without a prefix (prefix_bits 0) there is one histogram, got ", P,
                                    " prefixes"));
    // (the prefixes travel as kernel arguments: a device tensor is read back first)
    at::Tensor prefixes = prefixes0.cpu().contiguous();
    c10::hip::HIPGuard guard(col.device().index());
    hipStream_t s = c10::hip::getCurrentHIPStream(col.device().index()).stream();
    at::Tensor hist = pool_empty({P, 256}, col.options().dtype(at::kLong));
    k::select_hist(from_scalar_type(col.scalar_type()), col.data_ptr(), col.size(0), prefixes.data_ptr<int64_t>(),
                   static_cast<int>(P), prefix_bits, hist.data_ptr<int64_t>(), s);
    return hist;
  }, py::arg("col"), py::arg("prefixes"), py::arg("prefix_bits"),
     "one step of a radix select over a dense scalar device column: int64 [P, 256], hist[p][d] = rows whose "
     "order-preserving word has its top prefix_bits bits (0, 8, ..., 56) equal to those of prefixes[p] and whose "
     "next 8-bit digit is d; exact counts");
  // GroupedData.agg / DataFrame.agg on device-resident columns (kernels/group_stats.hip)
  m.def("group_chunk_rows", [] { return k::group_chunk_rows(); }, "rows per work item of group_moments");
  // int64 device records [*, C, 6], contiguous
  auto group_records = [](const char* what, const at::Tensor& t) {
    if (!t.is_cuda()) throw py::value_error(str_cat(what, ": the records must be a device tensor"));
    if (t.scalar_type() != at::kLong) throw py::type_error(str_cat(what, ": the records must be int64 bit patterns"));
    if (t.dim() != 3 || t.size(2) != k::kGroupRecordFields || t.size(1) < 1 || t.size(1) > k::kMaxPackCols)
      throw py::value_error(str_cat(what, ": records [*, 1..", k::kMaxPackCols, ", ", k::kGroupRecordFields,
                                    "] expected"));
    if (!t.is_contiguous()) throw py::value_error(str_cat(what, ": the records are not contiguous"));
  };
  auto group_index = [](const char* what, const char* which, const at::Tensor& t, const at::Device& dev) {
    if (t.scalar_type() != at::kLong) throw py::type_error(str_cat(what, ": ", which, " must be int64"));
    if (!t.is_cuda() || t.device() != dev)
      throw py::value_error(str_cat(what, ": ", which, " must be a tensor on the columns' device"));
    if (t.dim() != 1) throw py::value_error(str_cat(what, ": ", which, " must be 1-D"));
    if (!t.is_contiguous()) throw py::value_error(str_cat(what, ": ", which, " is not contiguous"));
  };
  m.def("group_moments", [group_index](const std::vector<at::Tensor>& cols, const at::Tensor& perm,
                                       const at::Tensor& offsets) {
    const k::StatCols sc = stat_cols_from("group_moments", cols);
    const auto dev = cols[0].device();
    group_index("group_moments", "perm", perm, dev);
    group_index("group_moments", "offsets", offsets, dev);
    const int64_t n = cols[0].size(0), C = sc.n;
    if (perm.size(0) != n)
      throw py::value_error(str_cat("group_moments: perm has ", perm.size(0), " entries, the columns ", n, " rows"));
    if (offsets.size(0) < 1) throw py::value_error("group_moments: offsets [nseg + 1] expected, got none");
    const int64_t nseg = offsets.size(0) - 1;
    if (n == 0 || nseg == 0) {  // nothing is launched: empty records
      at::Tensor rec = at::zeros({nseg, C, k::kGroupRecordFields}, at::kLong);
      if (nseg) rec.select(2, 4).fill_(-1);  // (all ones)
      return rec.to(dev);
    }
    c10::hip::HIPGuard guard(dev.index());
    hipStream_t s = c10::hip::getCurrentHIPStream(dev.index()).stream();
    at::Tensor rec = pool_empty({nseg, C, k::kGroupRecordFields}, cols[0].options().dtype(at::kLong));
    const size_t wsb = k::group_moments_workspace_bytes(sc.n, n, nseg);
    at::Tensor ws = pool_empty({static_cast<int64_t>((wsb + 7) / 8)}, cols[0].options().dtype(at::kLong));
    {
      py::gil_scoped_release nogil;
      k::group_moments(sc, n, perm.data_ptr<int64_t>(), n, offsets.data_ptr<int64_t>(), nseg, rec.data_ptr<int64_t>(),
                       ws.data_ptr(), static_cast<size_t>(ws.numel()) * 8, s);
    }
    return rec;
  }, py::arg("cols"), py::arg("perm"), py::arg("offsets"),
     "up to 16 dense scalar device columns [n] (mixed dtypes, contiguous) and segment_csr's (perm [n], offsets "
     "[nseg + 1]) -> int64 records [nseg, C, 6] (bit patterns): n, mean, M2 as f64, the sum (wrapping int64 for "
     "integer columns, f64 for float ones), the smallest and largest order-preserving word. A record depends on its "
     "segment's rows in row order alone; the same bits on every run. One stream synchronisation reads the number of "
     "work items; n == 0 launches nothing and gives empty records (0, 0, 0, 0, all ones, 0)");
  m.def("merge_group_records", [group_records, group_index](const at::Tensor& recs, const at::Tensor& offsets,
                                                            const std::vector<bool>& is_float) {
    group_records("merge_group_records", recs);
    group_index("merge_group_records", "offsets", offsets, recs.device());
    const int64_t mm = recs.size(0), C = recs.size(1);
    if (static_cast<int64_t>(is_float.size()) != C)
      throw py::value_error(str_cat("merge_group_records: ", C, " record columns, ", is_float.size(), " float flags"));
    if (offsets.size(0) < 1) throw py::value_error("merge_group_records: offsets [ng + 1] expected, got none");
    const int64_t ng = offsets.size(0) - 1;
    uint32_t mask = 0;
    for (int64_t c = 0; c < C; ++c) mask |= is_float[c] ? (1u << c) : 0u;
    c10::hip::HIPGuard guard(recs.device().index());
    hipStream_t s = c10::hip::getCurrentHIPStream(recs.device().index()).stream();
    at::Tensor out = pool_empty({ng, C, k::kGroupRecordFields}, recs.options());
    k::merge_group_records(mm ? recs.data_ptr<int64_t>() : nullptr, mm, static_cast<int>(C), mask,
                           offsets.data_ptr<int64_t>(), ng, out.data_ptr<int64_t>(), s);
    return out;
  }, py::arg("records"), py::arg("offsets"), py::arg("is_float"),
     "records [m, C, 6] ordered by (key, partition) and CSR offsets [ng + 1] over them -> [ng, C, 6]: each group's "
     "records merged in order with Chan's formula (integer sums add, float sums add in that order, words take min "
     "and max); is_float[c]: column c is float32 / float64");
  m.def("group_results", [group_records](const at::Tensor& recs, const std::vector<int64_t>& cols,
                                         const std::vector<std::string>& stats,
                                         const std::vector<at::ScalarType>& dtypes) {
    static const char* const names[] = {"count", "sum", "avg", "min", "max", "var_samp", "var_pop", "stddev_samp",
                                        "stddev_pop"};
    group_records("group_results", recs);
    const int64_t ng = recs.size(0), C = recs.size(1);
    if (cols.empty() || cols.size() > static_cast<size_t>(k::kMaxPackCols))
      throw py::value_error(str_cat("group_results: 1..", k::kMaxPackCols, " outputs per call, got ", cols.size()));
    if (stats.size() != cols.size() || dtypes.size() != cols.size())
      throw py::value_error("group_results: one statistic and one column dtype per output expected");
    k::GroupResultSpec spec;
    spec.n = static_cast<int>(cols.size());
    c10::hip::HIPGuard guard(recs.device().index());
    std::vector<at::Tensor> outs;
    for (size_t o = 0; o < cols.size(); ++o) {
      if (cols[o] < 0 || cols[o] >= C)
        throw py::value_error(str_cat("group_results: output ", o, " names column ", cols[o], " of ", C));
      const int st = name_index(names, stats[o]);
      if (st < 0) throw py::value_error(str_cat("group_results: '", stats[o], "' is not a statistic"));
      const at::ScalarType ct = dtypes[o];
      require_stat_type(ct, str_cat("group_results: output ", o, " reads a "), " column");
      const bool fl = ct == at::kFloat || ct == at::kDouble;
      const auto gs = static_cast<k::GroupStat>(st);
      at::ScalarType ot = at::kDouble;
      if (gs == k::GroupStat::COUNT || (gs == k::GroupStat::SUM && !fl)) ot = at::kLong;
      if (gs == k::GroupStat::MIN || gs == k::GroupStat::MAX) ot = ct;
      outs.push_back(pool_empty({ng}, recs.options().dtype(ot)));
      spec.col[o] = static_cast<int>(cols[o]);
      spec.stat[o] = gs;
      spec.dtype[o] = from_scalar_type(ct);
      spec.out[o] = outs.back().data_ptr();
    }
    k::group_results(ng ? recs.data_ptr<int64_t>() : nullptr, ng, static_cast<int>(C), spec,
                     c10::hip::getCurrentHIPStream(recs.device().index()).stream());
    return outs;
  }, py::arg("records"), py::arg("cols"), py::arg("stats"), py::arg("dtypes"),
     "merged records [ng, C, 6] -> one device column [ng] per output (up to 16, one launch): output o is statistic "
     "stats[o] (count, sum, avg, min, max, var_samp, var_pop, stddev_samp, stddev_pop) of record column cols[o], whose "
     "values have dtype dtypes[o]. count and integer sums are int64, min / max the column's dtype (words decoded: "
     "-0.0 comes back as 0.0), the others float64; a NaN or opposite infinities in a float group give NaN, the "
     "sample statistics NaN below two rows");
  // corr / covar_samp / covar_pop on device-resident columns (kernels/stats.hip, kernels/group_stats.hip)
  // xs[q], ys[q]: 1..kMaxPackCols pairs, all columns on one device and of one length
  auto pair_cols_from = [](const char* what, const std::vector<at::Tensor>& xs, const std::vector<at::Tensor>& ys,
                           k::StatCols* sx, k::StatCols* sy) {
    if (xs.size() != ys.size())
      throw py::value_error(str_cat(what, ": ", xs.size(), " first columns, ", ys.size(), " second columns"));
    if (xs.empty() || xs.size() > static_cast<size_t>(k::kMaxPackCols))
      throw py::value_error(str_cat(what, ": 1..", k::kMaxPackCols, " pairs per call, got ", xs.size()));
    *sx = stat_cols_from(what, xs);
    *sy = stat_cols_from(what, ys);
    if (ys[0].device() != xs[0].device())
      throw py::value_error(str_cat(what, ": the second columns are not on the first columns' device"));
    if (ys[0].size(0) != xs[0].size(0))
      throw py::value_error(str_cat(what, ": the second columns have ", ys[0].size(0), " rows, the first columns ",
                                    xs[0].size(0)));
  };
  // int64 device pair records [*, Q, 7], contiguous
  auto pair_records = [](const char* what, const at::Tensor& t) {
    if (!t.is_cuda()) throw py::value_error(str_cat(what, ": the records must be a device tensor"));
    if (t.scalar_type() != at::kLong) throw py::type_error(str_cat(what, ": the records must be int64 bit patterns"));
    if (t.dim() != 3 || t.size(2) != k::kPairRecordFields || t.size(1) < 1 || t.size(1) > k::kMaxPackCols)
      throw py::value_error(str_cat(what, ": records [*, 1..", k::kMaxPackCols, ", ", k::kPairRecordFields,
                                    "] expected"));
    if (!t.is_contiguous()) throw py::value_error(str_cat(what, ": the records are not contiguous"));
  };
  m.def("column_pair_moments", [pair_cols_from](const std::vector<at::Tensor>& xs, const std::vector<at::Tensor>& ys) {
    k::StatCols sx, sy;
    pair_cols_from("column_pair_moments", xs, ys, &sx, &sy);
    const int64_t n = xs[0].size(0), Q = sx.n;
    const auto dev = xs[0].device();
    if (n == 0) return at::zeros({Q, k::kPairRecordFields}, at::kLong).to(dev);  // nothing is launched
    c10::hip::HIPGuard guard(dev.index());
    hipStream_t s = c10::hip::getCurrentHIPStream(dev.index()).stream();
    at::Tensor rec = pool_empty({Q, k::kPairRecordFields}, xs[0].options().dtype(at::kLong));
    const size_t wsb = k::column_pair_moments_workspace_bytes(sx.n, n);
    at::Tensor ws = pool_empty({static_cast<int64_t>((wsb + 7) / 8)}, xs[0].options().dtype(at::kLong));
    k::column_pair_moments(sx, sy, n, rec.data_ptr<int64_t>(), ws.data_ptr(), static_cast<size_t>(ws.numel()) * 8, s);
    return rec;
  }, py::arg("xs"), py::arg("ys"),
     "up to 16 pairs (xs[q], ys[q]) of dense scalar device columns [n] (mixed dtypes, contiguous; a column may appear "
     "in several pairs) -> int64 records [Q, 7] (bit patterns): n, mean_x, mean_y, M2_x, M2_y, C_xy = sum (x - mean_x)"
     "(y - mean_y) as f64 and the count of rows whose x or y is NaN or an infinity; the same bits on every run. "
     "n == 0 launches nothing and gives empty records (all zeros)");
  m.def("group_pair_moments", [pair_cols_from, group_index](const std::vector<at::Tensor>& xs,
                                                            const std::vector<at::Tensor>& ys, const at::Tensor& perm,
                                                            const at::Tensor& offsets) {
    k::StatCols sx, sy;
    pair_cols_from("group_pair_moments", xs, ys, &sx, &sy);
    const auto dev = xs[0].device();
    group_index("group_pair_moments", "perm", perm, dev);
    group_index("group_pair_moments", "offsets", offsets, dev);
    const int64_t n = xs[0].size(0), Q = sx.n;
    if (perm.size(0) != n)
      throw py::value_error(str_cat("group_pair_moments: perm has ", perm.size(0), " entries, the columns ", n,
                                    " rows"));
    if (offsets.size(0) < 1) throw py::value_error("group_pair_moments: offsets [nseg + 1] expected, got none");
    const int64_t nseg = offsets.size(0) - 1;
    if (n == 0 || nseg == 0) return at::zeros({nseg, Q, k::kPairRecordFields}, at::kLong).to(dev);
    c10::hip::HIPGuard guard(dev.index());
    hipStream_t s = c10::hip::getCurrentHIPStream(dev.index()).stream();
    at::Tensor rec = pool_empty({nseg, Q, k::kPairRecordFields}, xs[0].options().dtype(at::kLong));
    const size_t wsb = k::group_pair_moments_workspace_bytes(sx.n, n, nseg);
    at::Tensor ws = pool_empty({static_cast<int64_t>((wsb + 7) / 8)}, xs[0].options().dtype(at::kLong));
    {
      py::gil_scoped_release nogil;
      k::group_pair_moments(sx, sy, n, perm.data_ptr<int64_t>(), n, offsets.data_ptr<int64_t>(), nseg,
                            rec.data_ptr<int64_t>(), ws.data_ptr(), static_cast<size_t>(ws.numel()) * 8, s);
    }
    return rec;
  }, py::arg("xs"), py::arg("ys"), py::arg("perm"), py::arg("offsets"),
     "up to 16 pairs (xs[q], ys[q]) of dense scalar device columns [n] and segment_csr's (perm [n], offsets "
     "[nseg + 1]) -> int64 pair records [nseg, Q, 7] (column_pair_moments' fields). group_moments' work items; a "
     "record depends on its segment's rows in row order alone. n == 0 launches nothing and gives empty records");
  m.def("group_both_moments", [pair_cols_from, group_index](const std::vector<at::Tensor>& cols,
                                                            const std::vector<at::Tensor>& xs,
                                                            const std::vector<at::Tensor>& ys, const at::Tensor& perm,
                                                            const at::Tensor& offsets) {
    const k::StatCols sc = stat_cols_from("group_both_moments", cols);
    k::StatCols sx, sy;
    pair_cols_from("group_both_moments", xs, ys, &sx, &sy);
    const auto dev = cols[0].device();
    const int64_t n = cols[0].size(0), C = sc.n, Q = sx.n;
    if (xs[0].device() != dev || xs[0].size(0) != n)
      throw py::value_error("group_both_moments: the pair columns are not on the columns' device or of their length");
    group_index("group_both_moments", "perm", perm, dev);
    group_index("group_both_moments", "offsets", offsets, dev);
    if (perm.size(0) != n)
      throw py::value_error(str_cat("group_both_moments: perm has ", perm.size(0), " entries, the columns ", n,
                                    " rows"));
    if (offsets.size(0) < 1) throw py::value_error("group_both_moments: offsets [nseg + 1] expected, got none");
    const int64_t nseg = offsets.size(0) - 1;
    if (n == 0 || nseg == 0) {
      at::Tensor rec = at::zeros({nseg, C, k::kGroupRecordFields}, at::kLong);
      if (nseg) rec.select(2, 4).fill_(-1);  // (all ones)
      return py::make_tuple(rec.to(dev), at::zeros({nseg, Q, k::kPairRecordFields}, at::kLong).to(dev));
    }
    c10::hip::HIPGuard guard(dev.index());
    hipStream_t s = c10::hip::getCurrentHIPStream(dev.index()).stream();
    const auto opts = cols[0].options().dtype(at::kLong);
    at::Tensor rec = pool_empty({nseg, C, k::kGroupRecordFields}, opts);
    at::Tensor prec = pool_empty({nseg, Q, k::kPairRecordFields}, opts);
    const size_t ib = k::group_items_workspace_bytes(nseg);
    const size_t wa = k::group_moments_workspace_bytes(sc.n, n, nseg);
    const size_t wb = k::group_pair_moments_workspace_bytes(sx.n, n, nseg);
    at::Tensor wi = pool_empty({static_cast<int64_t>((ib + 7) / 8)}, opts);
    at::Tensor ws = pool_empty({static_cast<int64_t>((std::max(wa, wb) + 7) / 8)}, opts);
    {
      py::gil_scoped_release nogil;
      // the work items are built once; both passes run in stream order and share the workspace of partial records
      const k::GroupItems items = k::group_items(offsets.data_ptr<int64_t>(), nseg, n, wi.data_ptr(),
                                                 static_cast<size_t>(wi.numel()) * 8, s);
      k::group_moments(sc, n, perm.data_ptr<int64_t>(), n, offsets.data_ptr<int64_t>(), nseg, rec.data_ptr<int64_t>(),
                       ws.data_ptr(), static_cast<size_t>(ws.numel()) * 8, s, &items);
      k::group_pair_moments(sx, sy, n, perm.data_ptr<int64_t>(), n, offsets.data_ptr<int64_t>(), nseg,
                            prec.data_ptr<int64_t>(), ws.data_ptr(), static_cast<size_t>(ws.numel()) * 8, s, &items);
    }
    return py::make_tuple(rec, prec);
  }, py::arg("cols"), py::arg("xs"), py::arg("ys"), py::arg("perm"), py::arg("offsets"),
     "group_moments(cols, perm, offsets) and group_pair_moments(xs, ys, perm, offsets) of one CSR -> (records "
     "[nseg, C, 6], pair records [nseg, Q, 7]), the same bits as the two calls; the work items (chunk counts and "
     "their scan, one stream synchronisation) are built once for both");
  m.def("merge_pair_records", [pair_records, group_index](const at::Tensor& recs, const at::Tensor& offsets) {
    pair_records("merge_pair_records", recs);
    group_index("merge_pair_records", "offsets", offsets, recs.device());
    const int64_t mm = recs.size(0), Q = recs.size(1);
    if (offsets.size(0) < 1) throw py::value_error("merge_pair_records: offsets [ng + 1] expected, got none");
    const int64_t ng = offsets.size(0) - 1;
    c10::hip::HIPGuard guard(recs.device().index());
    hipStream_t s = c10::hip::getCurrentHIPStream(recs.device().index()).stream();
    at::Tensor out = pool_empty({ng, Q, k::kPairRecordFields}, recs.options());
    k::merge_pair_records(mm ? recs.data_ptr<int64_t>() : nullptr, mm, static_cast<int>(Q),
                          offsets.data_ptr<int64_t>(), ng, out.data_ptr<int64_t>(), s);
    return out;
  }, py::arg("records"), py::arg("offsets"),
     "pair records [m, Q, 7] ordered by (key, partition) and CSR offsets [ng + 1] over them -> [ng, Q, 7]: each "
     "group's records merged in order with Chan's formula (the non-finite counts add)");
  m.def("pair_results", [pair_records](const at::Tensor& recs, const std::vector<int64_t>& pairs,
                                       const std::vector<std::string>& stats) {
    static const char* const names[] = {"corr", "covar_samp", "covar_pop"};
    pair_records("pair_results", recs);
    const int64_t ng = recs.size(0), Q = recs.size(1);
    if (pairs.empty() || pairs.size() > static_cast<size_t>(k::kMaxPackCols))
      throw py::value_error(str_cat("pair_results: 1..", k::kMaxPackCols, " outputs per call, got ", pairs.size()));
    if (stats.size() != pairs.size()) throw py::value_error("pair_results: one statistic per output expected");
    k::PairResultSpec spec;
    spec.n = static_cast<int>(pairs.size());
    c10::hip::HIPGuard guard(recs.device().index());
    std::vector<at::Tensor> outs;
    for (size_t o = 0; o < pairs.size(); ++o) {
      if (pairs[o] < 0 || pairs[o] >= Q)
        throw py::value_error(str_cat("pair_results: output ", o, " names pair ", pairs[o], " of ", Q));
      const int st = name_index(names, stats[o]);
      if (st < 0) throw py::value_error(str_cat("pair_results: '", stats[o], "' is not a pair statistic"));
      outs.push_back(pool_empty({ng}, recs.options().dtype(at::kDouble)));
      spec.pair[o] = static_cast<int>(pairs[o]);
      spec.stat[o] = static_cast<k::PairStat>(st);
      spec.out[o] = outs.back().data_ptr<double>();
    }
    k::pair_results(ng ? recs.data_ptr<int64_t>() : nullptr, ng, static_cast<int>(Q), spec,
                    c10::hip::getCurrentHIPStream(recs.device().index()).stream());
    return outs;
  }, py::arg("records"), py::arg("pairs"), py::arg("stats"),
     "merged pair records [ng, Q, 7] -> one float64 device column [ng] per output (up to 16, one launch): output o is "
     "stats[o] (corr, covar_samp, covar_pop) of pair pairs[o]. covar_pop = C / n (NaN without rows), covar_samp = "
     "C / (n - 1) (NaN below two rows), corr = C / sqrt(M2_x * M2_y) (NaN without rows or where an M2 is 0, not "
     "clamped); NaN where the record counts a row with a NaN or an infinity");
  // Window / .over() on device-resident partitions (kernels/window_scan.hip)
  m.def("window_tile_rows", [] { return k::window_tile_rows(); }, "rows per tile of window_scan");
  // int64 device bit patterns [rows, n], contiguous
  auto window_table = [](const char* what, const char* which, const at::Tensor& t) {
    if (!t.is_cuda()) throw py::value_error(str_cat(what, ": ", which, " must be a device tensor"));
    if (t.scalar_type() != at::kLong) throw py::type_error(str_cat(what, ": ", which, " must be int64 bit patterns"));
    if (t.dim() != 2) throw py::value_error(str_cat(what, ": ", which, " must be 2-D [*, n]"));
    if (!t.is_contiguous()) throw py::value_error(str_cat(what, ": ", which, " is not contiguous"));
  };
  m.def("window_scan", [window_table](const at::Tensor& words, int64_t P, bool reverse,
                                      const std::vector<std::string>& kinds, const std::vector<at::Tensor>& cols) {
    static const char* const names[] = {"group_head", "peer_head", "peer_count", "sum_i64", "sum_f64", "min_word",
                                        "max_word"};
    window_table("window_scan", "the words", words);
    const int64_t W = words.size(0), n = words.size(1);
    if (W > k::kMaxSortKeys)
      throw py::value_error(str_cat("window_scan: at most ", k::kMaxSortKeys, " words per row, got ", W));
    if (P < 0 || P > W) throw py::value_error(str_cat("window_scan: 0 <= P <= ", W, " expected, got ", P));
    if (kinds.empty() || kinds.size() > static_cast<size_t>(k::kMaxPackCols))
      throw py::value_error(str_cat("window_scan: 1..", k::kMaxPackCols, " channels per call, got ", kinds.size()));
    k::WindowChans ch;
    ch.n = static_cast<int>(kinds.size());
    size_t used = 0;
    for (size_t c = 0; c < kinds.size(); ++c) {
      const int kd = name_index(names, kinds[c]);
      if (kd < 0) throw py::value_error(str_cat("window_scan: '", kinds[c], "' is not a channel kind"));
      ch.kind[c] = kd;
      ch.dtype[c] = DType::U8;
      ch.ptr[c] = nullptr;
      if (kd < static_cast<int>(k::WindowChan::SUM_I64)) continue;
      if (used >= cols.size())
        throw py::value_error(str_cat("window_scan: channel ", c, " (", kinds[c], ") has no value column"));
      stat_column_like("window_scan", cols[used++], str_cat("the column of channel ", c), "the words", words.device(), n,
                       &ch.dtype[c], &ch.ptr[c]);
    }
    if (used != cols.size())
      throw py::value_error(str_cat("window_scan: ", cols.size(), " value columns for ", used, " value channels"));
    const int64_t C = ch.n;
    if (n == 0) return at::empty({C, 0}, words.options());  // nothing is launched
    c10::hip::HIPGuard guard(words.device().index());
    hipStream_t s = c10::hip::getCurrentHIPStream(words.device().index()).stream();
    at::Tensor out = pool_empty({C, n}, words.options());
    const size_t wsb = k::window_scan_workspace_bytes(ch.n, n);
    at::Tensor ws = pool_empty({static_cast<int64_t>((wsb + 7) / 8)}, words.options());
    k::window_scan(W ? words.data_ptr<int64_t>() : nullptr, static_cast<int>(W), static_cast<int>(P), n, reverse, ch,
                   out.data_ptr<int64_t>(), ws.data_ptr(), static_cast<size_t>(ws.numel()) * 8, s);
    return out;
  }, py::arg("words"), py::arg("P"), py::arg("reverse"), py::arg("kinds"), py::arg("cols"),
     "the words [W, n] of one sorted partition (int64 device bit patterns; the first P define groups, all W peers) "
     "-> int64 [C, n]: one segmented inclusive scan per channel kind (group_head, peer_head: the head's row index; "
     "peer_count; sum_i64, sum_f64, min_word, max_word of the next value column in cols). reverse scans the "
     "mirrored rows: the index channels give the last row of the group / peer run. Three launches, no block waits "
     "for another; the same bits on every run. n == 0 launches nothing");
  m.def("window_finish", [window_table](const at::Tensor& fwd, const at::Tensor& rev,
                                        const std::vector<std::string>& kinds, const std::vector<int64_t>& carry,
                                        const std::vector<int64_t>& total, bool has_carry, bool has_total,
                                        int64_t carry_rows, int64_t total_rows, const std::vector<std::string>& fns,
                                        const std::vector<std::string>& frames, const std::vector<int64_t>& chans,
                                        const std::vector<at::ScalarType>& dtypes) {
    static const char* const kind_names[] = {"group_head", "peer_head", "peer_count", "sum_i64", "sum_f64",
                                             "min_word", "max_word"};
    static const char* const fn_names[] = {"row_number", "rank", "dense_rank", "count", "sum", "avg", "min", "max"};
    static const char* const frame_names[] = {"rows", "range", "whole"};
    window_table("window_finish", "the forward scan", fwd);
    window_table("window_finish", "the reverse scan", rev);
    const int64_t C = fwd.size(0), n = fwd.size(1);
    if (rev.device() != fwd.device()) throw py::value_error("window_finish: the two scans are on different devices");
    if (rev.size(0) != 2 || rev.size(1) != n)
      throw py::value_error(str_cat("window_finish: a reverse scan [2, ", n, "] expected, got [", rev.size(0), ", ",
                                    rev.size(1), "]"));
    if (C < 2 || C > k::kMaxPackCols || static_cast<int64_t>(kinds.size()) != C ||
        static_cast<int64_t>(carry.size()) != C || static_cast<int64_t>(total.size()) != C)
      throw py::value_error(str_cat("window_finish: a forward scan of 2..", k::kMaxPackCols, " channels with one "
                                    "kind, carry and total each expected, got ", C, " channels, ", kinds.size(),
                                    " kinds, ", carry.size(), " carries, ", total.size(), " totals"));
    if (fns.empty() || fns.size() > static_cast<size_t>(k::kMaxPackCols))
      throw py::value_error(str_cat("window_finish: 1..", k::kMaxPackCols, " outputs per call, got ", fns.size()));
    if (frames.size() != fns.size() || chans.size() != fns.size() || dtypes.size() != fns.size())
      throw py::value_error("window_finish: one frame, channel and column dtype per output expected");
    if (carry_rows < 0 || total_rows < 0) throw py::value_error("window_finish: negative row count");
    k::WindowFinishSpec sp;
    sp.n_chan = static_cast<int>(C);
    std::vector<int> kd(C, -1);
    for (int64_t c = 0; c < C; ++c) {
      kd[c] = name_index(kind_names, kinds[c]);
      if (kd[c] < 0) throw py::value_error(str_cat("window_finish: '", kinds[c], "' is not a channel kind"));
      sp.op[c] = k::window_chan_op(kd[c]);
      sp.carry[c] = static_cast<uint64_t>(carry[c]);
      sp.total[c] = static_cast<uint64_t>(total[c]);
    }
    if (kd[0] != 0 || kd[1] != 1)
      throw py::value_error("window_finish: channels 0 and 1 of the forward scan must be group_head and peer_head");
    sp.has_carry = has_carry ? 1 : 0;
    sp.has_total = has_total ? 1 : 0;
    sp.carry_rows = carry_rows;
    sp.total_rows = total_rows;
    sp.n_out = static_cast<int>(fns.size());
    c10::hip::HIPGuard guard(fwd.device().index());
    std::vector<at::Tensor> outs;
    for (size_t o = 0; o < fns.size(); ++o) {
      const int fn = name_index(fn_names, fns[o]), fr = name_index(frame_names, frames[o]);
      if (fn < 0) throw py::value_error(str_cat("window_finish: '", fns[o], "' is not a window function"));
      if (fr < 0) throw py::value_error(str_cat("window_finish: '", frames[o], "' is not a frame"));
      if (chans[o] < 0 || chans[o] >= C)
        throw py::value_error(str_cat("window_finish: output ", o, " names channel ", chans[o], " of ", C));
      const at::ScalarType ct = dtypes[o];
      require_stat_type(ct, str_cat("window_finish: output ", o, " reads a "), " column");
      const auto wf = static_cast<k::WindowFn>(fn);
      const int ck = kd[chans[o]];
      at::ScalarType ot = at::kInt;
      bool fits = true;
      switch (wf) {
        case k::WindowFn::ROW_NUMBER:
        case k::WindowFn::RANK: break;
        case k::WindowFn::DENSE_RANK: fits = ck == 2; break;
        case k::WindowFn::COUNT: ot = at::kLong; break;
        case k::WindowFn::SUM: fits = ck == 3 || ck == 4; ot = ck == 3 ? at::kLong : at::kDouble; break;
        case k::WindowFn::AVG: fits = ck == 4; ot = at::kDouble; break;
        case k::WindowFn::MIN: fits = ck == 5; ot = ct; break;
        default: fits = ck == 6; ot = ct; break;  // MAX
      }
      if (!fits)
        throw py::value_error(str_cat("window_finish: output ", o, " (", fns[o], ") cannot read a ",
                                      kinds[chans[o]], " channel"));
      outs.push_back(pool_empty({n}, fwd.options().dtype(ot)));
      sp.fn[o] = wf;
      sp.frame[o] = static_cast<k::WindowFrame>(fr);
      sp.chan[o] = static_cast<int>(chans[o]);
      sp.dtype[o] = from_scalar_type(ct);
      sp.out[o] = outs.back().data_ptr();
    }
    if (n == 0) return outs;  // nothing is launched
    k::window_finish(fwd.data_ptr<int64_t>(), rev.data_ptr<int64_t>(), n, sp,
                     c10::hip::getCurrentHIPStream(fwd.device().index()).stream());
    return outs;
  }, py::arg("fwd"), py::arg("rev"), py::arg("kinds"), py::arg("carry"), py::arg("total"), py::arg("has_carry"),
     py::arg("has_total"), py::arg("carry_rows"), py::arg("total_rows"), py::arg("fns"), py::arg("frames"),
     py::arg("chans"), py::arg("dtypes"),
     "a forward window_scan [C, n] (channels 0, 1: group_head, peer_head; kinds names all C) and a reverse scan "
     "[2, n] of those two -> one device column [n] per output (up to 16, one launch): fns[o] (row_number, rank, "
     "dense_rank: int32; count: int64; sum: int64 or float64 as its channel; avg: float64; min, max: dtypes[o]) over "
     "frames[o] (rows, range, whole), read from channel chans[o]. carry[c] / carry_rows: the fold of the first "
     "group's pieces in earlier partitions, applied on the left when has_carry; total[c] / total_rows: the whole-"
     "group values of the last group when it runs on into a later partition (has_total)");
  // median / percentile / mode / countDistinct per group on device-resident partitions (kernels/group_order.hip)
  m.def("group_order_chunk_rows", [] { return k::group_order_chunk_rows(); },
        "rows per work item of group_order_summary");
  // the words [W, n] of one sorted partition and 0 <= P <= W <= kMaxSortKeys
  auto order_words = [window_table](const char* what, const at::Tensor& words, int64_t P) {
    window_table(what, "the words", words);
    const int64_t W = words.size(0);
    if (W > k::kMaxSortKeys)
      throw py::value_error(str_cat(what, ": at most ", k::kMaxSortKeys, " words per row, got ", W));
    if (P < 0 || P > W) throw py::value_error(str_cat(what, ": 0 <= P <= ", W, " expected, got ", P));
    if (words.size(1) >= (int64_t(1) << 31))
      throw py::value_error(str_cat(what, ": ", words.size(1), " rows; a partition of 2^31 rows or more does not fit"));
  };
  m.def("group_order_summary", [order_words](const at::Tensor& words, int64_t P) {
    order_words("group_order_summary", words, P);
    const int64_t W = words.size(0), n = words.size(1);
    const auto opts = words.options();
    if (n == 0)  // nothing is launched
      return py::make_tuple(at::zeros({1}, opts), at::empty({0}, opts), at::empty({0}, opts), at::empty({0}, opts));
    c10::hip::HIPGuard guard(words.device().index());
    hipStream_t s = c10::hip::getCurrentHIPStream(words.device().index()).stream();
    int64_t ng = 1;
    at::Tensor starts;
    if (P > 0) {
      const size_t ub = k::unique_workspace_bytes(n);
      at::Tensor uws = pool_empty({static_cast<int64_t>((ub + 7) / 8)}, opts);
      {
        py::gil_scoped_release nogil;
        ng = k::unique_plan(words.data_ptr<int64_t>(), static_cast<int>(P), n, nullptr, uws.data_ptr(),
                            uws.numel() * 8, s);
      }
      starts = pool_empty({ng + 1}, opts);
      k::unique_write(nullptr, n, ng, uws.data_ptr(), starts.data_ptr<int64_t>(), s);
    } else {
      starts = at::zeros({2}, opts);
    }
    starts.narrow(0, ng, 1).fill_(n);
    at::Tensor distinct = pool_empty({ng}, opts), mode_pos = pool_empty({ng}, opts), mode_len = pool_empty({ng}, opts);
    const size_t wsb = k::group_order_summary_workspace_bytes(n, ng);
    at::Tensor ws = pool_empty({static_cast<int64_t>((wsb + 15) / 16) * 2}, opts);
    {
      py::gil_scoped_release nogil;
      k::group_order_summary(W ? words.data_ptr<int64_t>() : nullptr, static_cast<int>(W), static_cast<int>(P), n,
                             starts.data_ptr<int64_t>(), ng, distinct.data_ptr<int64_t>(),
                             mode_pos.data_ptr<int64_t>(), mode_len.data_ptr<int64_t>(), ws.data_ptr(),
                             static_cast<size_t>(ws.numel()) * 8, s);
    }
    return py::make_tuple(starts, distinct, mode_pos, mode_len);
  }, py::arg("words"), py::arg("P"),
     "the words [W, n] of one sorted partition (int64 device bit patterns; the first P define groups, all W peer "
     "runs) -> (starts [ng + 1], distinct [ng], mode_pos [ng], mode_len [ng]), int64: the group heads in order with "
     "starts[ng] = n, the peer heads per group, and the head row and the length of the group's first longest peer "
     "run. A work item is at most group_order_chunk_rows() rows of one group; two stream synchronisations read the "
     "group and the work item counts. The same bytes on every run. n == 0 launches nothing");
  m.def("group_order_finish", [order_words](const at::Tensor& words, const at::Tensor& starts,
                                            const at::Tensor& distinct, const at::Tensor& mode_pos,
                                            const at::Tensor& mode_len, const std::vector<std::string>& fns,
                                            const std::vector<std::vector<double>>& percentages,
                                            at::ScalarType value_dtype) {
    static const char* const fn_names[] = {"count_distinct", "mode", "percentile_approx", "percentile"};
    order_words("group_order_finish", words, 0);
    const int64_t W = words.size(0), n = words.size(1);
    if (W < 1) throw py::value_error("group_order_finish: words [W, n] with W >= 1 expected; the last word is the value");
    auto vec = [&](const at::Tensor& t, const char* which, int64_t len) {
      if (!t.is_cuda() || t.device() != words.device())
        throw py::value_error(str_cat("group_order_finish: ", which, " must be a device tensor on the words' device"));
      if (t.scalar_type() != at::kLong)
        throw py::type_error(str_cat("group_order_finish: ", which, " must be int64, got ", c10::toString(t.scalar_type())));
      if (t.dim() != 1 || t.size(0) != len)
        throw py::value_error(str_cat("group_order_finish: ", which, " must hold [", len, "] entries, got ", t.dim(),
                                      "-D with ", t.numel()));
      if (!t.is_contiguous()) throw py::value_error(str_cat("group_order_finish: ", which, " is not contiguous"));
    };
    if (starts.dim() != 1 || starts.size(0) < 1)
      throw py::value_error("group_order_finish: starts [ng + 1] expected");
    const int64_t ng = starts.size(0) - 1;
    vec(starts, "starts", ng + 1);
    vec(distinct, "distinct", ng);
    vec(mode_pos, "mode_pos", ng);
    vec(mode_len, "mode_len", ng);
    if (ng > n) throw py::value_error(str_cat("group_order_finish: ", ng, " groups for ", n, " rows"));
    if ((ng == 0) != (n == 0)) throw py::value_error(str_cat("group_order_finish: ", ng, " groups for ", n, " rows"));
    if (fns.empty() || fns.size() > static_cast<size_t>(k::kMaxPackCols))
      throw py::value_error(str_cat("group_order_finish: 1..", k::kMaxPackCols, " outputs per call, got ", fns.size()));
    if (percentages.size() != fns.size())
      throw py::value_error("group_order_finish: one list of percentages per output expected (empty for mode and "
                            "count_distinct)");
    require_stat_type(value_dtype, "group_order_finish: the value column is a ", " column");
    k::GroupOrderSpec sp;
    sp.n_out = static_cast<int>(fns.size());
    sp.dtype = from_scalar_type(value_dtype);
    c10::hip::HIPGuard guard(words.device().index());
    std::vector<at::Tensor> outs;
    for (size_t o = 0; o < fns.size(); ++o) {
      const int fn = name_index(fn_names, fns[o]);
      if (fn < 0) throw py::value_error(str_cat("group_order_finish: '", fns[o], "' is not an order aggregate"));
      const auto gf = static_cast<k::GroupOrderFn>(fn);
      const bool ranked = gf == k::GroupOrderFn::PERCENTILE_APPROX || gf == k::GroupOrderFn::PERCENTILE;
      const auto& ps = percentages[o];
      if (ranked ? (ps.empty() || ps.size() > static_cast<size_t>(k::kMaxPercentages)) : !ps.empty())
        throw py::value_error(str_cat("group_order_finish: output ", o, " (", fns[o], ") takes ",
                                      ranked ? "1..16 percentages" : "no percentages", ", got ", ps.size()));
      for (double p : ps)
        if (!(p >= 0.0 && p <= 1.0))
          throw py::value_error(str_cat("group_order_finish: the percentage ", p, " is not in [0, 1]"));
      sp.fn[o] = gf;
      sp.nq[o] = ranked ? static_cast<int>(ps.size()) : 1;
      for (int q = 0; q < k::kMaxPercentages; ++q) sp.pct[o][q] = q < static_cast<int>(ps.size()) ? ps[q] : 0.0;
      const at::ScalarType ot = gf == k::GroupOrderFn::COUNT_DISTINCT ? at::kLong
                                : gf == k::GroupOrderFn::PERCENTILE   ? at::kDouble
                                                                      : value_dtype;
      // (a list of percentages gives [ng, Q]; the frame layer squeezes a single one)
      outs.push_back(ranked ? pool_empty({ng, static_cast<int64_t>(ps.size())}, words.options().dtype(ot))
                            : pool_empty({ng}, words.options().dtype(ot)));
      sp.out[o] = outs.back().data_ptr();
    }
    if (ng == 0) return outs;  // nothing is launched
    k::group_order_finish(words.data_ptr<int64_t>() + (W - 1) * n, n, starts.data_ptr<int64_t>(),
                          distinct.data_ptr<int64_t>(), mode_pos.data_ptr<int64_t>(), ng, sp,
                          c10::hip::getCurrentHIPStream(words.device().index()).stream());
    return outs;
  }, py::arg("words"), py::arg("starts"), py::arg("distinct"), py::arg("mode_pos"), py::arg("mode_len"),
     py::arg("fns"), py::arg("percentages"), py::arg("value_dtype"),
     "the words [W, n] of one sorted partition (the last word is the value) and group_order_summary's result -> one "
     "device tensor per output (up to 16, one launch): fns[o] of count_distinct (int64 [ng]), mode (value_dtype "
     "[ng]), percentile_approx (value_dtype [ng, Q]: the element at rank max(ceil(p N) - 1, 0)) or percentile "
     "(float64 [ng, Q]: Spark's linear interpolation, (hi - pos) v_lo + (pos - lo) v_hi without contraction), with "
     "percentages[o] its Q in 1..16 percentages in [0, 1] (empty for the first two)");
  // DataFrame.sample / randomSplit / sampleBy, F.rand / F.randn (kernels/random.hip)
  m.def("random_tile_rows", [] { return k::random_tile_rows(); }, "rows per block of the random_* kernels");
  // options of a [n] output on `device` (-1: the current one), after the checks every draw shares
  auto random_options = [](const char* what, int64_t row0, int64_t n, int64_t device) {
    if (n < 0) throw py::value_error(str_cat(what, ": a row count >= 0 is expected, got ", n));
    if (row0 < 0) throw py::value_error(str_cat(what, ": a global row index >= 0 is expected, got ", row0));
    if (row0 > std::numeric_limits<int64_t>::max() - n)
      throw py::value_error(str_cat(what, ": row0 + n passes 2^63 (", row0, " + ", n, ")"));
    const int ndev = static_cast<int>(c10::hip::device_count());
    if (ndev < 1) throw py::value_error(str_cat(what, ": no GPU is available"));
    if (device < -1 || device >= ndev)
      throw py::value_error(str_cat(what, ": device ", device, " does not exist (", ndev, " devices)"));
    const auto idx = static_cast<c10::DeviceIndex>(device < 0 ? c10::hip::current_device() : device);
    return at::TensorOptions().device(at::Device(at::kCUDA, idx));
  };
  m.def("random_uniform", [random_options](uint64_t seed, int64_t row0, int64_t n, int64_t device) {
    const auto opts = random_options("random_uniform", row0, n, device).dtype(at::kDouble);
    c10::hip::HIPGuard guard(opts.device().index());
    at::Tensor out = pool_empty({n}, opts);
    k::random_uniform(seed, static_cast<uint64_t>(row0), n, out.data_ptr<double>(),
                      c10::hip::getCurrentHIPStream(opts.device().index()).stream());
    return out;
  }, py::arg("seed"), py::arg("row0"), py::arg("n"), py::arg("device") = -1,
     "float64 [n] on the device: u of the rows row0 .. row0 + n of the Philox4x32-10 stream of `seed` (an unsigned "
     "64-bit key; counter (row low, row high, 0, 0)), u = (((w0 << 32) | w1) >> 11) * 2^-53 in [0, 1)");
  m.def("random_normal", [random_options](uint64_t seed, int64_t row0, int64_t n, int64_t device) {
    const auto opts = random_options("random_normal", row0, n, device).dtype(at::kDouble);
    c10::hip::HIPGuard guard(opts.device().index());
    at::Tensor out = pool_empty({n}, opts);
    k::random_normal(seed, static_cast<uint64_t>(row0), n, out.data_ptr<double>(),
                     c10::hip::getCurrentHIPStream(opts.device().index()).stream());
    return out;
  }, py::arg("seed"), py::arg("row0"), py::arg("n"), py::arg("device") = -1,
     "float64 [n]: the first Box-Muller normal of every row (counter word 2 is 1): sqrt(-2 ln u1) * cospi(2 u2), u1 "
     "from (w0, w1) in (0, 1], u2 from (w2, w3) in [0, 1)");
  m.def("random_mask", [random_options](uint64_t seed, int64_t row0, int64_t n, double lo, double hi,
                                        int64_t device) {
    const auto opts = random_options("random_mask", row0, n, device).dtype(at::kByte);
    if (std::isnan(lo) || std::isnan(hi))
      throw py::value_error(str_cat("random_mask: the bounds must be numbers, got ", lo, " and ", hi));
    c10::hip::HIPGuard guard(opts.device().index());
    at::Tensor out = pool_empty({n}, opts);
    k::random_mask(seed, static_cast<uint64_t>(row0), n, lo, hi, static_cast<uint8_t*>(out.data_ptr()),
                   c10::hip::getCurrentHIPStream(opts.device().index()).stream());
    return out;
  }, py::arg("seed"), py::arg("row0"), py::arg("n"), py::arg("lo"), py::arg("hi"), py::arg("device") = -1,
     "uint8 [n]: lo <= u < hi of every row's uniform draw (the byte mask compact_rows takes)");
  m.def("random_mask_by", [random_options](uint64_t seed, int64_t row0, const at::Tensor& words,
                                           const at::Tensor& table_words, const at::Tensor& table_fractions) {
    if (!words.is_cuda() || words.scalar_type() != at::kLong || words.dim() != 2 || words.size(0) != 1 ||
        !words.is_contiguous())
      throw py::value_error("random_mask_by: contiguous device int64 words [1, n] (sort_encode of one key) expected");
    const int64_t n = words.size(1);
    if (!table_words.is_cuda() || table_words.device() != words.device() || table_words.scalar_type() != at::kLong ||
        table_words.dim() != 1 || !table_words.is_contiguous())
      throw py::value_error("random_mask_by: a contiguous int64 word table [S] on the words' device expected");
    const int64_t S = table_words.size(0);
    if (S < 1 || S > k::kMaxStrata)
      throw py::value_error(str_cat("random_mask_by: 1..", k::kMaxStrata, " strata per call, got ", S));
    if (!table_fractions.is_cuda() || table_fractions.device() != words.device() ||
        table_fractions.scalar_type() != at::kDouble || table_fractions.dim() != 1 || table_fractions.size(0) != S ||
        !table_fractions.is_contiguous())
      throw py::value_error(str_cat("random_mask_by: a contiguous float64 fraction table [", S,
                                    "] on the words' device expected"));
    const auto opts = random_options("random_mask_by", row0, n, words.device().index()).dtype(at::kByte);
    c10::hip::HIPGuard guard(words.device().index());
    at::Tensor out = pool_empty({n}, opts);
    k::random_mask_by(seed, static_cast<uint64_t>(row0), n, words.data_ptr<int64_t>(), table_words.data_ptr<int64_t>(),
                      table_fractions.data_ptr<double>(), static_cast<int>(S), static_cast<uint8_t*>(out.data_ptr()),
                      c10::hip::getCurrentHIPStream(words.device().index()).stream());
    return out;
  }, py::arg("seed"), py::arg("row0"), py::arg("words"), py::arg("table_words"), py::arg("table_fractions"),
     "uint8 [n]: u < the fraction of the row's stratum. words [1, n]: sort_encode of the key column; table_words [S] "
     "ascending (as unsigned words) and distinct, table_fractions [S]; a word the table does not hold gives 0. At "
     "most 4096 strata (the table is staged in LDS)");
  m.def("random_poisson", [random_options](uint64_t seed, int64_t row0, int64_t n, const at::Tensor& cdf) {
    if (!cdf.is_cuda() || cdf.scalar_type() != at::kDouble || cdf.dim() != 1 || !cdf.is_contiguous())
      throw py::value_error("random_poisson: a contiguous device float64 table [len] expected");
    if (cdf.size(0) < 1 || cdf.size(0) > k::kMaxPoissonTable)
      throw py::value_error(str_cat("random_poisson: a table of 1..", k::kMaxPoissonTable, " entries, got ",
                                    cdf.size(0)));
    const auto opts = random_options("random_poisson", row0, n, cdf.device().index()).dtype(at::kLong);
    c10::hip::HIPGuard guard(cdf.device().index());
    at::Tensor out = pool_empty({n}, opts);
    k::random_poisson(seed, static_cast<uint64_t>(row0), n, cdf.data_ptr<double>(), static_cast<int>(cdf.size(0)),
                      out.data_ptr<int64_t>(), c10::hip::getCurrentHIPStream(cdf.device().index()).stream());
    return out;
  }, py::arg("seed"), py::arg("row0"), py::arg("n"), py::arg("cdf"),
     "int64 [n] on cdf's device: per row the number of entries of the non-decreasing table cdf [1..64] that are <= u "
     "(counter word 2 is 2): a Poisson count when cdf is the distribution function");
  m.def("random_expand", [](const at::Tensor& counts0) {
    if (!counts0.is_cuda() || counts0.scalar_type() != at::kLong || counts0.dim() != 1)
      throw py::value_error("random_expand: device int64 counts [n] expected");
    const int64_t n = counts0.size(0);
    c10::hip::HIPGuard guard(counts0.device().index());
    hipStream_t s = c10::hip::getCurrentHIPStream(counts0.device().index()).stream();
    at::Tensor counts = counts0.contiguous();
    at::Tensor offs = pool_empty({n + 1}, counts.options());
    int64_t total = 0;
    {
      const size_t wsb = k::join_scan_workspace_bytes(n);
      at::Tensor ws = pool_empty({static_cast<int64_t>((wsb + 7) / 8)}, counts.options());
      py::gil_scoped_release nogil;
      total = k::join_scan(counts.data_ptr<int64_t>(), n, k::kMaxPoissonTable, offs.data_ptr<int64_t>(), ws.data_ptr(),
                           static_cast<size_t>(ws.numel()) * 8, s);
    }
    at::Tensor idx = pool_empty({total}, counts.options());
    k::random_expand(offs.data_ptr<int64_t>(), n, total, idx.data_ptr<int64_t>(), s);
    return idx;
  }, py::arg("counts"),
     "random_poisson's counts [n] (each 0..64) -> int64 [sum]: row i counts[i] times, rows in order (the exclusive "
     "scan of join_expand, the left indices only; feeds take_rows); one stream synchronisation reads the total");
  // native JPEG decode into one ragged (pinned) buffer (runtime/jpeg_decode.cpp)
  struct PyJpegBatch {
    std::vector<py::buffer_info> views;  // keep the cells' buffers exported while decoding
    std::unique_ptr<tfa::JpegBatch> job;
    ~PyJpegBatch() { job.reset(); }  // waits for the tasks before the views go
  };
  py::class_<PyJpegBatch>(m, "JpegBatch")
      .def(py::init([](const py::list& cells, int channels, int threads, bool pinned) {
             TFA_CHECK(channels == 1 || channels == 3, "JpegBatch: channels must be 1 or 3");
             auto b = std::make_unique<PyJpegBatch>();
             std::vector<std::pair<const uint8_t*, size_t>> ptrs;
             b->views.reserve(cells.size());
             for (auto c : cells) {
               b->views.push_back(py::reinterpret_borrow<py::buffer>(c).request());
               const auto& v = b->views.back();
               ptrs.emplace_back(static_cast<const uint8_t*>(v.ptr), static_cast<size_t>(v.size * v.itemsize));
             }
             b->job = std::make_unique<tfa::JpegBatch>(std::move(ptrs), channels, threads, pinned);
             return b;
           }),
           py::arg("cells"), py::arg("channels"), py::arg("threads"), py::arg("pinned") = true)
      .def_property_readonly("header_ok", [](const PyJpegBatch& b) { return b.job->header_ok(); })
      .def_property_readonly("bad_header", [](const PyJpegBatch& b) { return b.job->bad_header(); })
      .def("wait", [](PyJpegBatch& b) {
        py::gil_scoped_release nogil;
        return b.job->wait();
      }, "block until every image is decoded; returns the indices that failed")
      .def_property_readonly("buffer", [](const PyJpegBatch& b) { return b.job->buffer(); })
      .def_property_readonly("meta_bytes", [](const PyJpegBatch& b) { return b.job->meta_bytes(); })
      .def_property_readonly("offsets_bytes", [](const PyJpegBatch& b) { return b.job->offsets_bytes(); })
      .def("shape", [](const PyJpegBatch& b, int64_t i) { return b.job->shape(i); })
      .def("pixel_offset", [](const PyJpegBatch& b, int64_t i) { return b.job->pixel_offset(i); });
  m.def("jpeg_native_available", [] {
    std::string why;
    bool ok = tfa::jpeg_native_available(&why);
    return py::make_tuple(ok, why);
  });
  m.def("set_step_timing", &tfa::set_step_timing, py::arg("on"),
        "time every step of GPU plan runs (a hipEvent pair each) until turned off");
  m.def("read_step_timing", [] {
    py::list out;
    for (const auto& r : tfa::read_step_timing()) {
      py::dict d;
      d["node"] = r.node;
      d["op"] = r.op;
      d["label"] = r.label;
      d["flops"] = r.flops;
      d["bytes"] = r.bytes;
      d["ms"] = r.ms;
      out.append(d);
    }
    return out;
  }, "wait for and drain the step records: [{node, op, label, flops, ms}] in launch order");
  m.def("roctx_push", [](const std::string& name) { roctxRangePushA(name.c_str()); }, py::arg("name"),
        "open a roctx range (rocprofv3 --marker-trace)");
  m.def("roctx_pop", [] { roctxRangePop(); });
  m.def("jpeg_native_info", [] {
    tfa::JpegLibInfo i = tfa::jpeg_native_info();
    py::dict d;
    d["ok"] = i.ok;
    d["version"] = i.version;
    d["struct_size"] = i.struct_size;
    d["soname"] = i.soname;
    d["why"] = i.why;
    return d;
  }, "the loaded libjpeg: its own version and decompressor size, and whether that layout is a known one");
  m.def("jpeg_force_version", &tfa::jpeg_force_version, py::arg("version"),
        "tests: treat the loaded libjpeg as this version (0 = its real one); unknown layouts disable the native path");
  m.def("jpeg_decode", [](const py::buffer& data, int channels) {
    auto v = data.request();
    tfa::JpegHeader h;
    const auto* p = static_cast<const uint8_t*>(v.ptr);
    size_t n = static_cast<size_t>(v.size * v.itemsize);
    TFA_CHECK(tfa::jpeg_parse_header(p, n, &h), "jpeg_decode: not a supported JPEG");
    at::Tensor out = at::empty({h.height, h.width, channels}, at::kByte);
    std::string err;
    bool ok;
    {
      py::gil_scoped_release nogil;
      ok = tfa::jpeg_decode_into(p, n, channels, out.data_ptr<uint8_t>(), out.numel(), &err);
    }
    TFA_CHECK(ok, "jpeg_decode: ", err);
    return out;
  }, py::arg("data"), py::arg("channels") = 3, "decode one JPEG on the calling thread (tests, tools)");
  m.def("decode_pool_threads", &tfa::decode_pool_threads);
  m.def("ragged_image_prep", [](const at::Tensor& data, const at::Tensor& offs, const at::Tensor& hw, int C, int OH,
                                 int OW, int mode, int oy, int ox, int h, int w,
                                 const std::vector<std::pair<int, std::vector<float>>>& ops,
                                 std::optional<at::Tensor> row_params) {
    // the batched map_rows image pre-stage (kernels/image.hip ragged_prep_kernel)
    TFA_CHECK(data.is_cuda() && data.scalar_type() == at::kByte && data.dim() == 1 && data.is_contiguous(),
              "ragged_image_prep: data must be a contiguous uint8 device buffer");
    const int64_t n = offs.numel();
    TFA_CHECK(offs.is_cuda() && offs.scalar_type() == at::kLong && offs.is_contiguous() && hw.is_cuda() &&
                  hw.scalar_type() == at::kInt && hw.is_contiguous() && hw.numel() == 2 * n,
              "ragged_image_prep: offsets int64 [n] and hw int32 [n, 2] device tensors expected");
    TFA_CHECK(ops.size() <= 4, "ragged_image_prep: at most 4 elementwise steps");
    k::RaggedPrepArgs a;
    a.n = n; a.C = C; a.OH = OH; a.OW = OW; a.mode = mode; a.oy = oy; a.ox = ox; a.h = h; a.w = w;
    a.nops = static_cast<int>(ops.size());
    for (size_t q = 0; q < ops.size(); ++q) {
      TFA_CHECK(ops[q].first >= 0 && ops[q].first <= 3,
                "ragged_image_prep: step kind must be 0 add, 1 sub, 2 mul, 3 div");
      const auto& v = ops[q].second;
      TFA_CHECK(v.size() == 1 || static_cast<int>(v.size()) == C, "ragged_image_prep: step constant of ", v.size(),
                " values for ", C, " channels");
      a.op_kind[q] = ops[q].first;
      a.op_chan[q] = v.size() > 1;
      for (size_t c = 0; c < v.size(); ++c) a.op_val[q][c] = v[c];
    }
    c10::hip::HIPGuard guard(data.device().index());
    at::Tensor rp;
    if (row_params) {
      // per-row (OH, OW, oy, ox): checked here on the host copy (the kernel
      // trusts them), then copied to the device on the stream
      const at::Tensor& hp = *row_params;
      TFA_CHECK(!hp.is_cuda() && hp.scalar_type() == at::kInt && hp.is_contiguous() && hp.numel() == 4 * n,
                "ragged_image_prep: row_params must be a host int32 [n, 4] tensor");
      const int32_t* p = hp.data_ptr<int32_t>();
      for (int64_t r = 0; r < n; ++r) {
        const int32_t RH = p[4 * r], RW = p[4 * r + 1], py = p[4 * r + 2], px = p[4 * r + 3];
        TFA_CHECK(RH > 0 && RW > 0 && py >= 0 && px >= 0 && py + h <= RH && px + w <= RW, "ragged_image_prep: row ",
                  r, ": crop ", h, "x", w, " at (", py, ", ", px, ") outside its ", RH, "x", RW, " resize");
      }
      rp = pool_empty({n, 4}, data.options().dtype(at::kInt));
      rp.copy_(hp, /*non_blocking=*/hp.is_pinned());
      a.rp = rp.data_ptr<int32_t>();
    }
    at::Tensor y = pool_empty({n, h, w, C}, data.options().dtype(at::kFloat));
    a.x = data.data_ptr<uint8_t>();
    a.offs = offs.data_ptr<int64_t>();
    a.hw = hw.data_ptr<int32_t>();
    a.y = y.data_ptr<float>();
    k::ragged_image_prep(a, c10::hip::getCurrentHIPStream(data.device().index()).stream());
    return y;
  }, py::arg("data"), py::arg("offsets"), py::arg("hw"), py::arg("channels"), py::arg("resize_h"),
        py::arg("resize_w"), py::arg("mode"), py::arg("crop_y"), py::arg("crop_x"), py::arg("crop_h"),
        py::arg("crop_w"), py::arg("ops"), py::arg("row_params") = py::none(),
        "n ragged uint8 HWC images -> f32 [n, crop_h, crop_w, C]: bilinear resize, crop, elementwise steps");
  m.def("gather_rows", [](const at::Tensor& x0, const at::Tensor& idx) {
    TFA_CHECK(x0.is_cuda() && idx.is_cuda() && idx.scalar_type() == at::kLong, "gather_rows: device tensors");
    c10::hip::HIPGuard guard(x0.device().index());
    at::Tensor x = x0.contiguous();
    auto sizes = x.sizes().vec();
    sizes[0] = idx.size(0);
    at::Tensor out = pool_empty(sizes, x.options());
    const int64_t inner = x.size(0) ? x.numel() / x.size(0) : 0;
    if (out.numel())
      k::gather(x.element_size(), DType::I64, x.data_ptr(), idx.contiguous().data_ptr(), out.data_ptr(), 1, x.size(0),
                idx.size(0), inner, c10::hip::getCurrentHIPStream(x.device().index()).stream());
    return out;
  }, "out[j] = x[idx[j]] along dim 0 (device gather kernel)");
  register_packer(m);
  register_pyencode(m);
  m.def("jit_compile", [](const std::string& src) { return jit::compile_only(src); },
        "compile a generated kernel with hiprtc for gfx950 (no device needed); returns the code-object size");
  m.def("jit_stats", []() {
    auto s = jit::stats();
    py::dict d;
    d["compiled"] = s.compiled;
    d["disk_hits"] = s.disk_hits;
    d["memory_hits"] = s.memory_hits;
    d["compile_ms"] = s.compile_ms;
    return d;
  });
  m.def("fusible_ops", [] {
    py::dict d;
    for (auto& o : tfa::fusible_ops()) {
      py::dict e;
      e["kind"] = std::string(o.kind);
      e["float_only"] = o.float_only;
      d[py::str(o.op)] = e;
    }
    return d;
  }, "every op the fusion generator can emit: name -> {kind: unary | binary | cast | view | broadcast, float_only}");
  m.def("set_fusion_index64", [](py::object on) { tfa::set_fusion_index64(!on.is_none() && on.cast<bool>()); },
        py::arg("on"),
        "True: every generated fusion kernel of a plan made from now on indexes with 64 bits, whatever its size "
        "(elementwise regions and row reductions); None or False: the automatic choice (64-bit from 2^31 elements). "
        "Read at planning time. The setting is part of the key of each program's plan cache, so a plan made under "
        "one setting is not served under the other; the generated sources differ, so the kernel cache needs nothing.");
  m.def("set_debug_sync", &set_debug_sync, "synchronise + check after every kernel (read per launch)");
  m.def("get_debug_sync", &get_debug_sync);
  m.def("f32_precision", [] { return k::f32_precision(); });
  m.def("set_gemm_tile", [](int cfg) { k::set_gemm_tile(cfg); });
  m.def("set_conv_smallc", [](bool on) { k::set_conv_smallc(on ? 1 : 0); },
        "route tiny-reduction convs (KH*KW*C <= 32) to the direct kernel (default on)");
  m.def("set_pool_conv_fusion", [](bool on) { tfa::set_pool_conv_fusion(on); }, py::arg("on"),
        "fuse a 3x3 VALID MaxPool into the 1x1 conv that alone reads it (GPU plans made after the call; default on)");
  m.def("set_conv_direct", [](bool on) { k::set_conv_direct(on ? 1 : 0); },
        "route narrow wide-image convs (C in {32, 64}, OC <= 64) to the direct LDS-filter kernel (default on)");
  m.def("set_conv_wino", [](bool on) { k::set_conv_wino(on ? 1 : 0); },
        "Winograd F(2x2,3x3) / F(2,7) for 3x3 / 1x7 / 7x1 stride-1 convs with constant filters (default on; TFA_CONV_ALGO=direct "
        "turns it off). Plans built while it is off carry no Winograd filters.");
  m.def("conv_wino_enabled", [] { return k::conv_wino_enabled(); });
  m.def("set_wino_5x5", [](bool on) { k::set_wino_5x5(on ? 1 : 0); }, py::arg("on"),
        "Winograd F(4,5) for 5x5 stride-1 convs in plans made after the call (opt-in)");
  m.def("set_wino_bn", &tfa::k::set_wino_bn, py::arg("bn"), "F(2x2,3x3) oc block: 0 auto (32 for OC <= 32), 32 or 64");
  m.def("set_wino_tile", [](int v) { k::set_wino_tile(v); },
        "force the Winograd kernel variant: -1 auto, 0 = 64 tiles x 64 oc, 1 = 128 tiles x 32 oc");
  m.def("conv_wino_filter", [](const at::Tensor& w) {
          TFA_CHECK(w.dim() == 4 && w.scalar_type() == at::kFloat, "conv_wino_filter: HWIO float32 filter");
          const int kind = k::conv_wino_kind(w.size(0), w.size(1), 1, 1, 1, 1, w.size(2), w.size(3));
          TFA_CHECK(kind != 0, "conv_wino_filter: 3x3, 1x7, 7x1 or 5x5 with C % 8 == 0 and OC % 4 == 0");
          at::Tensor wc = w.cpu().contiguous();
          at::Tensor u = at::empty({k::conv_wino_filter_elems(kind, wc.size(2), wc.size(3))}, wc.options());
          k::conv_wino_filter(kind, wc.data_ptr<float>(), wc.size(2), wc.size(3), u.data_ptr<float>());
          return u;
        }, "the planner's Winograd filter transform (fp64): 3x3 -> [C/8][16][2][OCP][4], 1x7 / 7x1 -> "
           "[C/8][8][2][OCP][4], flattened (tests)");
  m.def("gemm_tile_count", [] { return k::gemm_tile_count(); });
  m.def("gemm_tune_table", &k::gemm_tune_table, "the autotuner's tile picks: [(20-field shape key, tile)]");
  m.def("gemm_tune_seed", &k::gemm_tune_seed, py::arg("key"), py::arg("tile"),
        "a shipped default tile for a shape key (replaced only by a >= 2 % win confirmed twice)");
  m.def("gemm_tune_reset", &k::gemm_tune_reset, "forget the autotuner's picks (the defaults stay)");
  m.def("gemm_tile_dims", &k::gemm_tile_dims, py::arg("tile"), "{BM, BN, core}");
  m.def("roundtrip_graphdef",
        [](py::bytes b) { return py::bytes(serialize_graphdef(parse_graphdef(std::string(b)))); });
  m.def("decode_tensor_proto", [](py::bytes b) {
    HostTensor t = parse_tensor_proto(std::string(b));
    if (t.dtype == DType::STRING) {
      py::list l;
      for (auto& s : t.strings) l.append(py::bytes(s));
      return py::object(l);
    }
    return py::cast(host_tensor_to_at(t));
  });
  // Which kernels a reduction takes: the host-side routing of kernels/reduce.hip
  // (no device needed). The tests pin every case to the route it was written for.
  auto route_dtype = [](const std::string& name) {
    for (DType d : {DType::F32, DType::F64, DType::I32, DType::I64, DType::BOOL})
      if (name == dtype_name(d)) return d;
    TFA_CHECK(false, "reduce route: dtype ", name, " not supported (float32, float64, int32, int64, bool)");
    return DType::INVALID;
  };
  auto route_redop = [](const std::string& op) {
    k::RedOp rop = op == "Sum" ? k::RedOp::SUM : op == "Min" ? k::RedOp::MIN : op == "Max" ? k::RedOp::MAX
                 : op == "Prod" ? k::RedOp::PROD : k::RedOp::ALL;
    TFA_CHECK(rop != k::RedOp::ALL, "unsorted segment route: unsupported op ", op);
    return rop;
  };
  m.def("reduce_route", [route_dtype](const std::string& dtype, int64_t outer, int64_t r, int64_t inner, bool aligned16) {
    TFA_CHECK(outer > 0 && r > 0 && inner > 0, "reduce_route: outer, r and inner must be positive");
    return std::string(k::reduce_route_name(k::reduce_route(route_dtype(dtype), outer, r, inner, aligned16).route));
  }, py::arg("dtype"), py::arg("outer"), py::arg("r"), py::arg("inner"), py::arg("aligned16") = true,
     "name of the kernel route k::reduce takes for x viewed as [outer, r, inner]");
  m.def("reduce_route_info", [route_dtype](const std::string& dtype, int64_t outer, int64_t r, int64_t inner, bool aligned16) {
    TFA_CHECK(outer > 0 && r > 0 && inner > 0, "reduce_route: outer, r and inner must be positive");
    const DType dt = route_dtype(dtype);
    k::ReducePlan p = k::reduce_route(dt, outer, r, inner, aligned16);
    py::dict d;
    d["route"] = std::string(k::reduce_route_name(p.route));
    d["S"] = p.S;
    d["rows_per_split"] = p.rows_per_split;
    d["fold"] = p.fold;
    d["col_blocks"] = p.col_blocks;
    d["vec"] = p.vec;
    d["workspace_bytes"] = k::reduce_workspace_bytes(dt, outer, r, inner);
    return d;
  }, py::arg("dtype"), py::arg("outer"), py::arg("r"), py::arg("inner"), py::arg("aligned16") = true);
  m.def("reduce_route_names", [] {
    std::vector<std::string> v;
    for (int i = 0; i < (int)k::RedRoute::COUNT; ++i) v.push_back(k::reduce_route_name((k::RedRoute)i));
    return v;
  }, "every name reduce_route can return");
  // The host-side routing of kernels/gemm_f64.hip: f64 GEMM, integer GEMM, pooling.
  m.def("gemm_f64_route", [](int64_t M, int64_t N, int64_t K, int64_t batch, bool ta, bool tb, int64_t lda, int64_t ldb,
                             bool a_aligned16, bool b_aligned16) {
    TFA_CHECK(M > 0 && N > 0 && K >= 0 && batch > 0, "gemm_f64_route: M, N and batch must be positive");
    if (lda <= 0) lda = ta ? M : K;
    if (ldb <= 0) ldb = tb ? K : N;
    const k::GemmF64Plan p = k::gemm_f64_route(M, N, K, batch, ta, tb, lda, ldb, a_aligned16, b_aligned16);
    py::dict d;
    d["tile"] = std::string(k::gemm_f64_tile_name(p.tile));
    d["kernel"] = std::string(k::gemm_f64_tile_name(p.tile)) + (ta ? "_T" : "_N") + (tb ? "T" : "N");
    d["BM"] = p.BM;
    d["BN"] = p.BN;
    d["tiles_m"] = p.tiles_m;
    d["tiles_n"] = p.tiles_n;
    d["grid"] = py::make_tuple(p.tiles_m * p.tiles_n, 1, std::min(batch, k::kGemmMaxBatchPerLaunch));
    d["launches"] = p.launches;
    d["max_batch_per_launch"] = k::kGemmMaxBatchPerLaunch;
    d["k_mult16"] = p.k_mult16;
    d["a_pairs"] = p.a_pairs;
    d["b_pairs"] = p.b_pairs;
    return d;
  }, py::arg("M"), py::arg("N"), py::arg("K"), py::arg("batch") = 1, py::arg("ta") = false, py::arg("tb") = false,
     py::arg("lda") = 0, py::arg("ldb") = 0, py::arg("a_aligned16") = true, py::arg("b_aligned16") = true,
     "the launch k::gemm takes for a float64 GEMM (lda / ldb 0: the contiguous operand)");
  m.def("gemm_f64_kernel_names", [] {
    std::vector<std::string> v;
    for (int t = 0; t < (int)k::F64Tile::COUNT; ++t)
      for (const char* tr : {"_NN", "_NT", "_TN", "_TT"}) v.push_back(std::string(k::gemm_f64_tile_name((k::F64Tile)t)) + tr);
    return v;
  }, "every `kernel` gemm_f64_route can return: tile x transpose_a x transpose_b");
  m.def("gemm_int_route", [](int64_t M, int64_t N, int64_t K, int64_t batch) {
    TFA_CHECK(M > 0 && N > 0 && K >= 0 && batch > 0, "gemm_int_route: M, N and batch must be positive");
    const k::GemmIntPlan p = k::gemm_int_route(M, N, K, batch);
    py::dict d;
    d["tiles_m"] = p.tiles_m;
    d["tiles_n"] = p.tiles_n;
    d["grid"] = py::make_tuple(p.tiles_m * p.tiles_n, 1, std::min(batch, k::kGemmMaxBatchPerLaunch));
    d["launches"] = p.launches;
    d["max_batch_per_launch"] = k::kGemmMaxBatchPerLaunch;
    d["max_grid_x"] = (int64_t(1) << 31) - 1;
    return d;
  }, py::arg("M"), py::arg("N"), py::arg("K"), py::arg("batch") = 1,
     "the launch k::gemm takes for an int32 / int64 GEMM and the limits that apply");
  auto pool_plan = [](int64_t N, int64_t H, int64_t W, int64_t C, int64_t OH, int64_t OW, int64_t KH, int64_t KW,
                      int64_t ldc, bool x_aligned16, bool y_aligned16) {
    TFA_CHECK(N > 0 && H > 0 && W > 0 && C > 0 && OH > 0 && OW > 0 && KH > 0 && KW > 0 && ldc >= 0,
              "pool_route: sizes must be positive");
    k::PoolArgs a{};
    a.N = N; a.H = H; a.W = W; a.C = C; a.OH = OH; a.OW = OW; a.KH = KH; a.KW = KW; a.ldc = ldc;
    return k::pool_route(a, x_aligned16, y_aligned16);
  };
  m.def("pool_route", [pool_plan](int64_t N, int64_t H, int64_t W, int64_t C, int64_t OH, int64_t OW, int64_t KH,
                                  int64_t KW, int64_t ldc, bool x_aligned16, bool y_aligned16) {
    return std::string(k::pool_route_name(pool_plan(N, H, W, C, OH, OW, KH, KW, ldc, x_aligned16, y_aligned16).route));
  }, py::arg("N"), py::arg("H"), py::arg("W"), py::arg("C"), py::arg("OH"), py::arg("OW"), py::arg("KH"), py::arg("KW"),
     py::arg("ldc") = 0, py::arg("x_aligned16") = true, py::arg("y_aligned16") = true,
     "name of the kernel k::pool2d_nhwc takes (under TFA_POOL_GENERIC / TFA_POOL_XCD and set_pool_route)");
  m.def("pool_route_info", [pool_plan](int64_t N, int64_t H, int64_t W, int64_t C, int64_t OH, int64_t OW, int64_t KH,
                                       int64_t KW, int64_t ldc, bool x_aligned16, bool y_aligned16) {
    const k::PoolPlan p = pool_plan(N, H, W, C, OH, OW, KH, KW, ldc, x_aligned16, y_aligned16);
    py::dict d;
    d["route"] = std::string(k::pool_route_name(p.route));
    d["V"] = p.V;
    d["items"] = p.items;
    d["blocks"] = p.blocks;
    return d;
  }, py::arg("N"), py::arg("H"), py::arg("W"), py::arg("C"), py::arg("OH"), py::arg("OW"), py::arg("KH"), py::arg("KW"),
     py::arg("ldc") = 0, py::arg("x_aligned16") = true, py::arg("y_aligned16") = true);
  m.def("pool_route_names", [] {
    std::vector<std::string> v;
    for (int i = 0; i < (int)k::PoolRoute::COUNT; ++i) v.push_back(k::pool_route_name((k::PoolRoute)i));
    return v;
  }, "every name pool_route can return, from the most to the least specialised");
  m.def("set_pool_route", [](py::object route) {
    if (route.is_none()) return k::set_pool_route(-1);
    if (py::isinstance<py::str>(route)) {
      const std::string name = route.cast<std::string>();
      for (int i = 0; i < (int)k::PoolRoute::COUNT; ++i)
        if (name == k::pool_route_name((k::PoolRoute)i)) return k::set_pool_route(i);
      TFA_CHECK(false, "set_pool_route: unknown route ", name);
    }
    k::set_pool_route(route.cast<int>());
  }, py::arg("route"),
     "force a pool kernel process-wide (None or -1: automatic); only a less specialised route than the automatic one");
  m.def("unsorted_segment_route", [route_dtype, route_redop](const std::string& op, const std::string& dtype, int64_t n,
                                                             int64_t inner, int64_t nseg) {
    TFA_CHECK(n > 0 && inner > 0 && nseg > 0, "unsorted_segment_route: n, inner and nseg must be positive");
    return k::unsorted_segment_route_name(k::unsorted_segment_route(route_redop(op), route_dtype(dtype), n, inner, nseg));
  }, py::arg("op"), py::arg("dtype"), py::arg("n"), py::arg("inner"), py::arg("nseg"),
     "route of k::unsorted_segment_reduce: tiny_int, small_int, private_g<G>, sorted_perm_p<inner_pad>, sorted_perm_wide");
  m.def("unsorted_segment_route_info", [route_dtype, route_redop](const std::string& op, const std::string& dtype,
                                                                  int64_t n, int64_t inner, int64_t nseg) {
    TFA_CHECK(n > 0 && inner > 0 && nseg > 0, "unsorted_segment_route: n, inner and nseg must be positive");
    k::UsegPlan p = k::unsorted_segment_route(route_redop(op), route_dtype(dtype), n, inner, nseg);
    py::dict d;
    d["route"] = k::unsorted_segment_route_name(p);
    d["B"] = p.B;
    d["G"] = p.G;
    d["tile"] = p.tile;
    d["rows_per_block"] = p.rows_per_block;
    d["inner_pad"] = p.inner_pad;
    return d;
  }, py::arg("op"), py::arg("dtype"), py::arg("n"), py::arg("inner"), py::arg("nseg"));
  m.def("unsorted_segment_route_names", [] {
    std::vector<std::string> v{"tiny_int", "small_int"};
    for (int g = 1; g <= 64; g <<= 1) v.push_back("private_g" + std::to_string(g));
    for (int p = 1; p <= 64; p <<= 1) v.push_back("sorted_perm_p" + std::to_string(p));
    v.push_back("sorted_perm_wide");
    return v;
  }, "every name unsorted_segment_route can return");
  // Segmented reduction over rows sorted by segment (CSR offsets, int64):
  // the groupBy/aggregate monoid fast path. Device tensors run the HIP
  // kernel; host tensors the ATen reference.
  // Unsorted segmented reduction: out[ids[i]] op= x[i] (rows in any order),
  // the map-side combine of groupBy/aggregate. ids int32/int64 on x's device.
  m.def("unsorted_segment_reduce", [](const std::string& op, const at::Tensor& x, const at::Tensor& ids,
                                      int64_t nseg, std::optional<at::Tensor> out_opt) {
    TFA_CHECK(x.dim() >= 1 && ids.dim() == 1 && ids.size(0) == x.size(0), "unsorted_segment_reduce: ids must be [rows]");
    TFA_CHECK(ids.scalar_type() == at::kLong || ids.scalar_type() == at::kInt, "unsorted_segment_reduce: int ids");
    TFA_CHECK(ids.device() == x.device(), "unsorted_segment_reduce: ids and x on different devices");
    k::RedOp rop = op == "Sum" ? k::RedOp::SUM : op == "Min" ? k::RedOp::MIN : op == "Max" ? k::RedOp::MAX
                 : op == "Prod" ? k::RedOp::PROD : k::RedOp::ALL;
    TFA_CHECK(rop != k::RedOp::ALL, "unsorted_segment_reduce: unsupported op ", op);
    std::vector<int64_t> osz = x.sizes().vec();
    osz[0] = nseg;
    const int64_t nrows = x.size(0);
    if (!x.is_cuda()) {
      // the device kernels' rules: ids outside [0, nseg) are dropped, a segment
      // starts from the op's identity (Min / Max: the dtype's max() / lowest())
      int64_t cols = 1;
      for (int64_t i = 1; i < x.dim(); ++i) cols *= x.size(i);
      at::Tensor il = ids.to(at::kLong);
      at::Tensor valid = (il >= 0) & (il < nseg);
      at::Tensor xs = x.reshape({nrows, cols}).index({valid});
      at::Tensor is = il.index({valid});
      at::Tensor out;
      if (rop == k::RedOp::SUM) {
        out = at::zeros({nseg, cols}, x.options()).index_add_(0, is, xs);
      } else if (rop == k::RedOp::PROD) {
        out = at::ones({nseg, cols}, x.options()).index_reduce_(0, is, xs, "prod", true);
      } else {
        const bool mx = rop == k::RedOp::MAX;
        at::Scalar init;
        bool known = true;
        switch (x.scalar_type()) {
          case at::kInt: init = mx ? std::numeric_limits<int32_t>::lowest() : std::numeric_limits<int32_t>::max(); break;
          case at::kLong: init = mx ? std::numeric_limits<int64_t>::lowest() : std::numeric_limits<int64_t>::max(); break;
          case at::kFloat: init = mx ? std::numeric_limits<float>::lowest() : std::numeric_limits<float>::max(); break;
          case at::kDouble: init = mx ? std::numeric_limits<double>::lowest() : std::numeric_limits<double>::max(); break;
          default: known = false;  // a dtype the device kernels do not take: every segment must have a row
        }
        out = known ? at::full({nseg, cols}, init, x.options()) : at::empty({nseg, cols}, x.options());
        out = out.index_reduce_(0, is, xs, mx ? "amax" : "amin", known);
      }
      out = out.reshape(osz).contiguous();
      if (out_opt) return out_opt->copy_(out);
      return out;
    }
    c10::hip::HIPGuard guard(x.device().index());
    at::Tensor xc = x.contiguous(), ic = ids.contiguous();
    at::Tensor out;
    if (out_opt) {  // write into a caller's slice (e.g. one partition's row of a stacked buffer)
      out = *out_opt;
      TFA_CHECK(out.is_cuda() && out.is_contiguous() && out.sizes().vec() == osz && out.scalar_type() == xc.scalar_type(),
                "unsorted_segment_reduce: out must be a contiguous device tensor of the result shape and dtype");
    } else {
      out = pool_empty(osz, xc.options());
    }
    if (!out.numel()) return out;
    const int64_t inner = out.numel() / nseg;
    const DType dt = from_scalar_type(xc.scalar_type());
    size_t ws = k::unsorted_segment_workspace_bytes(rop, dt, nrows, inner, nseg);
    at::Tensor work;
    if (ws) work = pool_empty({static_cast<int64_t>(ws)}, xc.options().dtype(at::kByte));
    k::unsorted_segment_reduce(rop, dt, from_scalar_type(ic.scalar_type()), xc.data_ptr(), ic.data_ptr(),
                               out.data_ptr(), nrows, inner, nseg, ws ? work.data_ptr() : nullptr,
                               c10::hip::getCurrentHIPStream(x.device().index()).stream());
    return out;
  }, py::arg("op"), py::arg("x"), py::arg("ids"), py::arg("nseg"), py::arg("out") = py::none());
  m.def("segment_reduce", [](const std::string& op, const at::Tensor& x, const at::Tensor& offsets) {
    TFA_CHECK(x.dim() >= 1, "segment_reduce needs rank >= 1");
    TFA_CHECK(offsets.scalar_type() == at::kLong && offsets.dim() == 1, "offsets must be int64[nseg+1]");
    int64_t nseg = offsets.size(0) - 1;
    std::vector<int64_t> osz = x.sizes().vec();
    osz[0] = nseg;
    k::RedOp rop = op == "Sum" ? k::RedOp::SUM : op == "Min" ? k::RedOp::MIN : op == "Max" ? k::RedOp::MAX
                 : op == "Prod" ? k::RedOp::PROD : op == "Mean" ? k::RedOp::MEAN : k::RedOp::ALL;
    TFA_CHECK(rop != k::RedOp::ALL, "segment_reduce: unsupported op ", op);
    if (!x.is_cuda()) {
      at::Tensor off = offsets.to(at::kCPU);
      const int64_t* o = off.data_ptr<int64_t>();
      std::vector<at::Tensor> parts;
      for (int64_t s = 0; s < nseg; ++s) {
        at::Tensor seg = x.narrow(0, o[s], o[s + 1] - o[s]);
        switch (rop) {
          case k::RedOp::SUM: parts.push_back(seg.sum(0, false, x.scalar_type())); break;
          case k::RedOp::MIN: parts.push_back(std::get<0>(seg.min(0))); break;
          case k::RedOp::MAX: parts.push_back(std::get<0>(seg.max(0))); break;
          case k::RedOp::PROD: parts.push_back(seg.prod(0, false, x.scalar_type())); break;
          default: parts.push_back(seg.to(at::kDouble).mean(0).to(x.scalar_type()));
        }
      }
      return nseg ? at::stack(parts, 0) : at::empty(osz, x.options());
    }
    c10::hip::HIPGuard guard(x.device().index());
    at::Tensor xc = x.contiguous();
    at::Tensor out = pool_empty(osz, xc.options());
    int64_t inner = nseg ? out.numel() / nseg : 0;
    if (out.numel())
      k::segment_reduce_csr(rop, from_scalar_type(xc.scalar_type()), xc.data_ptr(),
                            offsets.contiguous().data_ptr<int64_t>(), out.data_ptr(), nseg, inner,
                            c10::hip::getCurrentHIPStream(x.device().index()).stream());
    return out;
  });
  m.def("empty_pinned", &empty_pinned);
  m.def("trim_pinned_pool", &trim_pinned_pool);
  m.def("is_pinned", [](const at::Tensor& t) {
    // torch's is_pinned() only knows its own host allocator; ask HIP directly
    if (t.is_cuda() || !t.numel()) return false;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, t.data_ptr()) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    return attr.type == hipMemoryTypeHost;
  });
  m.def("pinned_pool_cached_bytes", &pinned_pool_cached_bytes);
  m.def("device_pool_stats", [] {
    DevPoolStats v = dev_pool_stats();
    py::dict d;
    d["allocs"] = v.allocs;
    d["frees"] = v.frees;
    d["fallbacks"] = v.fallbacks;
    d["capture_allocs"] = v.capture_allocs;
    d["device_mallocs"] = v.device_mallocs;
    d["live"] = v.live_bytes;
    d["peak"] = v.peak_bytes;
    d["cached"] = v.cached_bytes;
    return d;
  }, "engine-owned device pool: allocations, frees, c10 fallbacks, HIP-graph capture allocations, hipMallocs, live / peak / cached bytes");
  m.def("trim_device_pool", &dev_pool_trim);
  // ---- engine-owned communicators (csrc/comm/comm.h)
  {
    using comm::Comm;
    using GR = py::call_guard<py::gil_scoped_release>;
    py::class_<Comm, std::shared_ptr<Comm>>(m, "Comm",
        "engine communicator: all_reduce / all_gather / all_to_all_v / broadcast on the current stream")
        .def_property_readonly("rank", &Comm::rank)
        .def_property_readonly("size", &Comm::size)
        .def_property_readonly("kind", &Comm::kind)
        .def_property_readonly("calls", &Comm::calls)
        .def("all_reduce", [](Comm& c, at::Tensor t, const std::string& op) {
          c.all_reduce(t, comm::parse_op(op));
          return t;
        }, py::arg("tensor"), py::arg("op") = "Sum", GR())
        .def("all_gather", &Comm::all_gather, GR())
        .def("all_to_all_v", &Comm::all_to_all_v, py::arg("x"), py::arg("send_rows"), py::arg("recv_rows"), GR())
        .def("broadcast", [](Comm& c, at::Tensor t, int root) {
          c.broadcast(t, root);
          return t;
        }, py::arg("tensor"), py::arg("root") = 0, GR())
        .def("barrier", &Comm::barrier, GR());
    py::class_<comm::FakeWorld, std::shared_ptr<comm::FakeWorld>>(m, "FakeWorld",
        "N in-process ranks over host memory (CPU test double of the communicator)")
        .def(py::init<int>())
        .def_property_readonly("size", &comm::FakeWorld::size)
        .def("comm", [](std::shared_ptr<comm::FakeWorld> w, int r) {
          return std::shared_ptr<Comm>(std::make_shared<comm::FakeComm>(w, r));
        });
    py::class_<comm::RcclComm, Comm, std::shared_ptr<comm::RcclComm>>(m, "RcclComm",
        "an RCCL communicator of the engine's own (ncclCommInitRank)")
        .def(py::init([](py::bytes uid, int rank, int size, int device) {
          std::string u = uid;
          py::gil_scoped_release nogil;
          return std::make_shared<comm::RcclComm>(u, rank, size, device);
        }), py::arg("unique_id"), py::arg("rank"), py::arg("size"), py::arg("device"))
        .def("abort", &comm::RcclComm::abort, GR())
        .def("async_error", &comm::RcclComm::async_error)
        .def("set_timeout", &comm::RcclComm::set_timeout, py::arg("seconds"), py::arg("exit_on_timeout") = true,
             "seconds a collective may take (<= 0: unbounded); past it wait() raises CollectiveError, and past it "
             "plus a grace period the watchdog thread aborts the communicator and exits the process "
             "(exit_on_timeout) or marks it failed")
        .def_property_readonly("timeout", &comm::RcclComm::timeout)
        .def("wait", &comm::RcclComm::wait, GR(), "bounded wait for every collective issued so far")
        .def("check", &comm::RcclComm::check, "raises CollectiveError if the communicator failed")
        .def_property_readonly("failed", &comm::RcclComm::failed)
        .def_property_readonly("inflight", &comm::RcclComm::inflight)
        .def("set_test_stall", &comm::RcclComm::set_test_stall, py::arg("seconds"),
             "tests: a spin kernel inside each all_reduce, after its start event");
    py::class_<comm::ShmComm, Comm, std::shared_ptr<comm::ShmComm>>(m, "ShmComm",
        "host tensors of the ranks of one node through a POSIX shared-memory segment")
        .def(py::init<const std::string&, int, int, int64_t, bool>(), py::arg("name"), py::arg("rank"),
             py::arg("size"), py::arg("slot_bytes"), py::arg("create"), GR())
        .def("unlink", &comm::ShmComm::unlink)
        .def("set_timeout", &comm::ShmComm::set_timeout, py::arg("seconds"))
        .def("poison", &comm::ShmComm::poison, "make every rank's current / next collective raise")
        .def("reset_after_failure", &comm::ShmComm::reset_after_failure,
             "clear the barrier state (only once every rank has left the communicator)")
        .def_property_readonly("poisoned", &comm::ShmComm::poisoned)
        .def_property_readonly("slot_bytes", &comm::ShmComm::slot_bytes)
        .def_property_readonly("attached", &comm::ShmComm::attached);
    m.attr("EXIT_COLLECTIVE_TIMEOUT") = comm::kExitCollectiveTimeout;
    m.def("device_stall", [](double seconds) {
      k::device_stall(static_cast<uint64_t>(std::max(0.0, seconds) * 1e6),
                      c10::hip::getCurrentHIPStream().stream());
    }, py::arg("seconds"), "fault injection: a bounded (<= 60 s) spin kernel on the current stream");
    m.def("can_access_peer", [](int a, int b) {
      int ok = 0;
      if (hipDeviceCanAccessPeer(&ok, a, b) != hipSuccess) {
        (void)hipGetLastError();
        return false;
      }
      return ok != 0;
    }, py::arg("device"), py::arg("peer"));
    m.def("rccl_unique_id", [] { return py::bytes(comm::rccl_unique_id()); });
    py::class_<comm::OneShotComm, std::shared_ptr<comm::OneShotComm>>(m, "OneShotComm",
        "single-hop all-reduce of payloads <= 64 KB through IPC-mapped peer buffers")
        .def(py::init<int, int, int>(), py::arg("rank"), py::arg("size"), py::arg("device"))
        .def("ipc_handle", [](comm::OneShotComm& o) { return py::bytes(o.ipc_handle()); })
        .def("open", &comm::OneShotComm::open)
        .def_property_readonly("ready", &comm::OneShotComm::ready)
        .def_property_readonly("calls", &comm::OneShotComm::calls)
        .def_static("max_bytes", &comm::OneShotComm::max_bytes)
        .def("all_reduce", [](comm::OneShotComm& o, at::Tensor t, const std::string& op) {
          o.all_reduce(t, comm::parse_op(op));
          return t;
        }, py::arg("tensor"), py::arg("op") = "Sum", GR())
        .def("check", &comm::OneShotComm::check, GR())
        .def("set_timeout", &comm::OneShotComm::set_timeout, py::arg("seconds"))
        .def_property_readonly("alloc_kind", &comm::OneShotComm::alloc_kind)
        .def_property_readonly("failed", &comm::OneShotComm::failed);
  }
  m.def("cat_rows", [](const std::vector<at::Tensor>& ts) {
    TFA_CHECK(!ts.empty(), "cat_rows: no tensors");
    const at::Tensor& t0 = ts[0];
    TFA_CHECK(t0.is_cuda() && t0.dim() >= 1, "cat_rows: device tensors of rank >= 1 expected");
    std::vector<int64_t> sz = t0.sizes().vec();
    int64_t rows = 0;
    for (auto& t : ts) {
      TFA_CHECK(t.is_cuda() && t.device() == t0.device() && t.scalar_type() == t0.scalar_type() &&
                    t.dim() == t0.dim() && t.sizes().slice(1) == t0.sizes().slice(1),
                "cat_rows: tensors must share device, dtype and trailing shape");
      rows += t.size(0);
    }
    sz[0] = rows;
    c10::hip::HIPGuard guard(t0.device().index());
    at::Tensor out = pool_empty(sz, t0.options());
    hipStream_t st = c10::hip::getCurrentHIPStream(t0.device().index()).stream();
    std::vector<at::Tensor> keep;  // contiguous copies of strided inputs, alive until launched
    k::CopyPieces pc;
    int64_t off = 0;
    auto flush = [&]() {
      k::batched_copy(pc, out.data_ptr(), st);
      pc.n = 0;
    };
    for (auto& t0i : ts) {
      at::Tensor t = t0i.is_contiguous() ? t0i : t0i.contiguous();
      if (!t0i.is_contiguous()) keep.push_back(t);
      const int64_t nb = t.numel() * t.element_size();
      if (nb) {
        pc.src[pc.n] = t.data_ptr();
        pc.dst_off[pc.n] = off;
        pc.bytes[pc.n] = nb;
        if (++pc.n == k::kMaxCopyPieces) flush();
      }
      off += nb;
    }
    flush();
    for (auto& t : keep) dev_record_stream(t, st);
    return out;
  }, py::arg("tensors"), "row concatenation of device tensors into one pool buffer: one batched-copy kernel");
  m.def("cat_rows_many", [](const std::vector<std::vector<at::Tensor>>& cols) {
    // several row concatenations (the columns of merged partitions) into ONE
    // pool buffer with one batched-copy launch per 32 pieces; each result is
    // a view of that buffer at a 256-byte aligned offset
    TFA_CHECK(!cols.empty() && !cols[0].empty(), "cat_rows_many: no tensors");
    const at::Tensor& t00 = cols[0][0];
    TFA_CHECK(t00.is_cuda(), "cat_rows_many: device tensors expected");
    std::vector<std::vector<int64_t>> shapes;
    std::vector<int64_t> offs;
    int64_t total = 0;
    for (auto& ts : cols) {
      TFA_CHECK(!ts.empty(), "cat_rows_many: empty column");
      const at::Tensor& t0 = ts[0];
      TFA_CHECK(t0.dim() >= 1, "cat_rows_many: tensors of rank >= 1 expected");
      std::vector<int64_t> sz = t0.sizes().vec();
      int64_t rows = 0, nb = 0;
      for (auto& t : ts) {
        TFA_CHECK(t.is_cuda() && t.device() == t00.device() && t.scalar_type() == t0.scalar_type() &&
                      t.dim() == t0.dim() && t.sizes().slice(1) == t0.sizes().slice(1),
                  "cat_rows_many: the tensors of a column must share device, dtype and trailing shape");
        rows += t.size(0);
        nb += t.numel() * t.element_size();
      }
      sz[0] = rows;
      shapes.push_back(sz);
      offs.push_back(total);
      total += (nb + 255) / 256 * 256;
    }
    c10::hip::HIPGuard guard(t00.device().index());
    at::Tensor buf = pool_empty({std::max<int64_t>(total, 1)}, t00.options().dtype(at::kByte));
    hipStream_t st = c10::hip::getCurrentHIPStream(t00.device().index()).stream();
    std::vector<at::Tensor> keep;
    k::CopyPieces pc;
    auto flush = [&]() {
      k::batched_copy(pc, buf.data_ptr(), st);
      pc.n = 0;
    };
    for (size_t c = 0; c < cols.size(); ++c) {
      int64_t off = offs[c];
      for (auto& t0i : cols[c]) {
        at::Tensor t = t0i.is_contiguous() ? t0i : t0i.contiguous();
        if (!t0i.is_contiguous()) keep.push_back(t);
        const int64_t nb = t.numel() * t.element_size();
        if (nb) {
          pc.src[pc.n] = t.data_ptr();
          pc.dst_off[pc.n] = off;
          pc.bytes[pc.n] = nb;
          if (++pc.n == k::kMaxCopyPieces) flush();
        }
        off += nb;
      }
    }
    flush();
    for (auto& t : keep) dev_record_stream(t, st);
    std::vector<at::Tensor> out;
    for (size_t c = 0; c < cols.size(); ++c) {
      const auto dt = cols[c][0].scalar_type();
      int64_t n = 1;
      for (int64_t d : shapes[c]) n *= d;
      out.push_back(buf.narrow(0, offs[c], n * c10::elementSize(dt)).view(dt).view(shapes[c]));
    }
    return out;
  }, py::arg("columns"), "row concatenations of several columns into one pool buffer (views of it)");
  m.def("pipeline_wait", &pipeline_wait, py::arg("handle"), py::call_guard<py::gil_scoped_release>(),
        "wait for a run_chunked(wait=False) completion handle (and release it)");
  // ---- zero-word packing of pipeline outputs (kernels/pack_words.hip, runtime/unpack.cpp)
  m.def("set_pack_outputs", &set_pack_outputs, py::arg("on"),
        "run_chunked packs eligible fetches before their D2H copy (config.pack_outputs)");
  m.def("pack_outputs", &pack_outputs);
  m.def("set_pack_dense_fraction", &set_pack_dense_fraction, py::arg("t"),
        "packed / dense size ratio above which a fetch goes back to plain copies (<= 0: the built-in value)");
  m.def("pack_dense_fraction", &pack_dense_fraction);
  m.def("pack_layout", [](int64_t rows, int64_t wpr) {
    const PackLayout L = pack_layout(rows, wpr);
    py::dict d;
    d["tile_rows"] = kPackTileRows;
    d["tiles"] = L.tiles;
    d["mask_words"] = L.mask_words;
    d["mask_off"] = L.mask_off;
    d["values_off"] = L.values_off;
    d["max_bytes"] = L.max_bytes;
    return d;
  }, py::arg("rows"), py::arg("wpr"), "byte layout of a packed rows x wpr buffer (kernels/pack_layout.h)");
  m.def("pack_words", [](const at::Tensor& src, int64_t rows, int64_t wpr) {
    TFA_CHECK(src.is_cuda() && src.is_contiguous(), "pack_words: contiguous device tensor expected");
    TFA_CHECK(rows >= 0 && wpr >= 0 && static_cast<int64_t>(src.numel() * src.element_size()) == rows * wpr * 4,
              "pack_words: the tensor is not ", rows, " x ", wpr, " words");
    c10::hip::HIPGuard guard(src.device().index());
    at::Tensor out = pool_empty({static_cast<int64_t>(k::pack_words_max_bytes(rows, wpr))},
                                at::TensorOptions().dtype(at::kByte).device(src.device()));
    k::pack_words(src.data_ptr(), rows, wpr, out.data_ptr(), c10::hip::getCurrentHIPStream(src.device().index()).stream());
    return out;
  }, py::arg("src"), py::arg("rows"), py::arg("wpr"),
        "the packed form (uint8 [max_bytes]; the first 8 bytes are the value word count) of a device buffer");
  m.def("unpack_words", [](const at::Tensor& packed, at::Tensor& out, int64_t rows, int64_t wpr, int threads) {
    TFA_CHECK(!packed.is_cuda() && !out.is_cuda() && packed.is_contiguous() && out.is_contiguous(),
              "unpack_words: contiguous host tensors expected");
    const PackLayout L = pack_layout(rows, wpr);
    const size_t have = packed.numel() * packed.element_size();
    TFA_CHECK(have >= L.values_off, "unpack_words: packed buffer shorter than its header and mask");
    const uint64_t total = rows && wpr ? *static_cast<const uint64_t*>(packed.data_ptr()) : 0;
    TFA_CHECK(total <= static_cast<uint64_t>(rows * wpr) && have >= L.values_off + total * 4,
              "unpack_words: packed buffer shorter than its ", total, " values");
    TFA_CHECK(static_cast<int64_t>(out.numel() * out.element_size()) == rows * wpr * 4,
              "unpack_words: the output is not ", rows, " x ", wpr, " words");
    py::gil_scoped_release nogil;
    if (threads <= 0) {
      unpack::unpack_buffer(packed.data_ptr(), out.data_ptr(), rows, wpr, 0, L.tiles);
    } else {
      unpack::Pool pool(threads);
      pool.post_unpack(packed.data_ptr(), out.data_ptr(), rows, wpr)->wait();
    }
  }, py::arg("packed"), py::arg("out"), py::arg("rows"), py::arg("wpr"), py::arg("threads") = 0,
        "expand a packed host buffer into `out` (threads > 0: on a pool of that many workers)");
  m.def("unpack_force_variant", &unpack::force_variant, py::arg("variant"),
        "test hook: -1 auto, 0 scalar, 1 AVX2, 2 AVX-512");
  m.def("unpack_variant_available", &unpack::variant_available, py::arg("variant"));
  m.def("unpack_current_variant", &unpack::current_variant);
  m.def("unpack_default_threads", &unpack::default_threads);
  m.def("unpack_pool_raise", [](int threads, int parts, int bad_part) {
    py::gil_scoped_release nogil;
    unpack::Pool pool(threads);
    pool.post(parts, [bad_part](int p) {
      if (p == bad_part) throw std::runtime_error("unpack pool test: part " + std::to_string(p) + " failed");
    })->wait();
  }, py::arg("threads"), py::arg("parts"), py::arg("bad_part"),
        "test hook: a pool job whose part `bad_part` throws; the waiter (this call) re-raises it");
  py::module_::import("atexit").attr("register")(py::cpp_function([] {
    py::gil_scoped_release nogil;
    shutdown_pack_runtime();
  }));
  m.def("device_empty", [](const std::vector<int64_t>& sizes, at::ScalarType dt, int device) {
    c10::hip::HIPGuard guard(static_cast<c10::DeviceIndex>(device));
    return pool_empty(sizes, at::TensorOptions().dtype(dt).device(at::kCUDA, static_cast<c10::DeviceIndex>(device)));
  }, py::arg("sizes"), py::arg("dtype"), py::arg("device"),
        "uninitialised device tensor from the engine pool, ordered on the device's current stream");
  m.def("device_zeros", [](const std::vector<int64_t>& sizes, at::ScalarType dt, int device) {
    c10::hip::HIPGuard guard(static_cast<c10::DeviceIndex>(device));
    return pool_zeros(sizes, at::TensorOptions().dtype(dt).device(at::kCUDA, static_cast<c10::DeviceIndex>(device)));
  }, py::arg("sizes"), py::arg("dtype"), py::arg("device"), "zeroed (hipMemsetAsync) device tensor from the engine pool");
  m.def("fill_", [](at::Tensor& t, double value) {
    TFA_CHECK(t.is_cuda() && t.is_contiguous(), "fill_: contiguous device tensor expected");
    c10::hip::HIPGuard guard(t.device().index());
    k::fill(from_scalar_type(t.scalar_type()), t.data_ptr(), t.numel(), value,
            c10::hip::getCurrentHIPStream(t.device().index()).stream());
    return t;
  }, py::arg("tensor"), py::arg("value"), "fill a device tensor in place (kernels/elementwise fill)");
  m.def("record_stream", [](const at::Tensor& t, uint64_t stream) {
    TFA_CHECK(t.is_cuda(), "record_stream: device tensor expected");
    dev_record_stream(t, reinterpret_cast<hipStream_t>(stream));
  }, py::arg("tensor"), py::arg("stream"),
        "the tensor is also used on `stream` (a hipStream_t handle): its memory (engine pool or c10) is not "
        "reused before that stream's work queued so far has finished");
  m.def("pinned_pool_stats", [] {
    auto v = pinned_pool_stats();
    py::dict d;
    d["limit"] = v[0];
    d["cached"] = v[1];
    d["live"] = v[2];
    d["peak"] = v[3];
    return d;
  }, "page-locked pool: cap, cached free bytes, live bytes, peak live bytes");
  m.def("pin_host_tensor", &pin_host_tensor);
  m.def("unpin_host_tensor", &unpin_host_tensor);
}
