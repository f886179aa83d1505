// pybind11 module `boom_amd._boom`: the slice of BayesBoom's `boom` module that
// sits on the spike-and-slab path, with the same names and call shapes as the
// reference's bindings (Interfaces/python/BayesBoom/Models/Glm/GlmModel_def.cpp:
// 787-828 BregVsSampler; RegressionModel, GlmCoefs; Models/Model_def.cpp
// MvnGivenScalarSigma / ChisqModel / VariableSelectionPrior;
// ModelWrapper.cpp:89-119 sample_posterior / set_method), so that the driver
// loop of Interfaces/python/spikeslab/BayesBoom/spikeslab/spikeslab.py:191-207
//
//     model = boom.RegressionModel(X, y, False)
//     sampler = boom.BregVsSampler(model, slab, siginv_prior, spike)
//     model.set_method(sampler)
//     model.coef.drop_all(); model.coef.add(0)
//     for i in range(niter):
//         model.sample_posterior(); record(model.sigma, model.coef)
//
// runs unchanged with `import boom_amd._boom as boom`.  Everything goes through
// the C++ host side (include/boom_amd.hpp) and from there the C-ABI: no compute
// happens in this file.  Extra keyword arguments (chains=, seed=, device=) and
// accessors (chain_states, set_lookahead) expose what is new: many chains.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include "boom_amd.hpp"

namespace py = pybind11;
using namespace boom_amd_api;

namespace {

typedef py::array_t<double, py::array::c_style | py::array::forcecast> NpArray;

Matrix matrix_from(const NpArray &a) {
  if (a.ndim() != 2) throw std::runtime_error("expected a 2-d array");
  Matrix m((int)a.shape(0), (int)a.shape(1));
  auto r = a.unchecked<2>();
  for (py::ssize_t i = 0; i < a.shape(0); ++i)
    for (py::ssize_t j = 0; j < a.shape(1); ++j) m((int)i, (int)j) = r(i, j);
  return m;
}
Vector vector_from(const NpArray &a) {
  // (c_style | forcecast: the data are contiguous doubles whatever the shape)
  const double *d = a.data();
  return Vector(d, d + a.size());
}
py::array_t<double> to_numpy(const Vector &v) {
  py::array_t<double> out((py::ssize_t)v.size());
  auto w = out.mutable_unchecked<1>();
  for (size_t i = 0; i < v.size(); ++i) w((py::ssize_t)i) = v[i];
  return out;
}
// a family's simulate_forecast (horizon x chains, column c = chain c) as chains x horizon
py::array_t<double> forecast_to_numpy(const Matrix &m) {
  py::array_t<double> out({(py::ssize_t)m.ncol(), (py::ssize_t)m.nrow()});
  auto w = out.mutable_unchecked<2>();
  for (int c = 0; c < m.ncol(); ++c)
    for (int i = 0; i < m.nrow(); ++i) w(c, i) = m(i, c);
  return out;
}
// a Matrix as it stands (rows x columns)
py::array_t<double> matrix_to_numpy(const Matrix &m) {
  py::array_t<double> out({(py::ssize_t)m.nrow(), (py::ssize_t)m.ncol()});
  auto w = out.mutable_unchecked<2>();
  for (int c = 0; c < m.ncol(); ++c)
    for (int i = 0; i < m.nrow(); ++i) w(i, c) = m(i, c);
  return out;
}
Vector optional_vector(const py::object &a) { return a.is_none() ? Vector() : vector_from(a.cast<NpArray>()); }

// what the models of the latent-data families (Poisson, logit) share; scale: a forecast's exposures or trials
template <class Model, class... Extra>
py::class_<Model, Extra...> latent_data_class(py::class_<Model, Extra...> cls, const char *scale, const char *forecast_doc) {
  return cls
      .def("latent_values", [](const Model &m, int chain) { return to_numpy(m.latent_values(chain)); },
           py::arg("chain") = 0, "the latent values of one chain (0 at a missing step)")
      .def("latent_precisions", [](const Model &m, int chain) { return to_numpy(m.latent_precisions(chain)); },
           py::arg("chain") = 0, "the latent values' precisions in one chain (0 at a missing step)")
      .def("set_latent_data", [](Model &m, const NpArray &value, const NpArray &precision, int chain) {
             m.set_latent_data(vector_from(value), vector_from(precision), chain);
           }, py::arg("value"), py::arg("precision"), py::arg("chain") = -1)
      .def("impute_state", &Model::impute_state)
      .def("simulate_forecast", [](Model &m, const NpArray &predictors, const py::object &scale) {
             return forecast_to_numpy(m.simulate_forecast(matrix_from(predictors), optional_vector(scale)));
           }, py::arg("predictors"), py::arg(scale) = py::none(), forecast_doc);
}

// GlmCoefs as the drivers use it: model.coef.drop_all() / add / inc / Beta
struct CoefView {
  RegressionModel *model;
};

// boom.BinomialLogitModel(xdim, include_all) / BinomialProbitModel, filled by
// add_dataset(successes, trials, predictors) as in BayesBoom (GlmModel_def.cpp:549-590).
// The reference's sampler reads the model's data at every draw; here the data go to
// the device once, when the sampler -- which brings clt_threshold -- is attached.
struct PyBinomialModel {
  int xdim;
  bool logit;
  int chains;
  uint64_t seed;
  int device;
  std::vector<uint8_t> inc;          // coef.inc until the device model exists
  Matrix X;
  Vector y, n;
  bool have_data = false;
  Ptr<BinomialRegressionModelBase> impl;

  PyBinomialModel(int xdim_, bool include_all, bool logit_, int chains_, uint64_t seed_, int device_)
      : xdim(xdim_), logit(logit_), chains(chains_), seed(seed_), device(device_),
        inc((size_t)xdim_, include_all ? 1 : 0) {
    if (xdim_ <= 0) throw std::runtime_error("xdim must be positive");
    if (!include_all) inc[0] = 1;    // "only the intercept starts out included"
  }
  void materialise(int clt_threshold) {
    if (!have_data) throw std::runtime_error("add_dataset(successes, trials, predictors) before attaching a sampler");
    // a sampler holds a raw pointer to the device model (as BOOM's samplers hold their
    // model): replacing it under a sampler already attached would leave that sampler
    // dangling, so the device model is created exactly once
    if (impl) throw std::runtime_error("a sampler has already been attached to this model: create a new model to change clt_threshold or the sampler");
    if (logit) impl.reset(new BinomialLogitModel(X, y, n, clt_threshold, chains, seed, device));
    else impl.reset(new BinomialProbitModel(X, y, n, clt_threshold, chains, seed, device));
    impl->drop_all();
    for (int j = 0; j < xdim; ++j)
      if (inc[j]) impl->add(j);
  }
  void need_impl() const {
    if (!impl) throw std::runtime_error("no sampler attached to the model yet");
  }
};
struct BinomialCoefView {
  PyBinomialModel *model;
};

template <class SamplerT, class ModelT>
Ptr<SamplerT> make_binomial_sampler(PyBinomialModel &m, const Ptr<MvnModel> &slab,
                                    const Ptr<VariableSelectionPrior> &spike, int clt_threshold) {
  m.materialise(clt_threshold);
  return Ptr<SamplerT>(new SamplerT(static_cast<ModelT *>(m.impl.get()), slab, spike));
}

template <class PyClass>
void bind_binomial_model(PyClass &c) {
  c.def("add_dataset",
        [](PyBinomialModel &m, const NpArray &successes, const NpArray &trials, const NpArray &predictors) {
          m.X = matrix_from(predictors);
          m.y = vector_from(successes);
          m.n = vector_from(trials);
          if (m.X.ncol() != m.xdim) throw std::runtime_error("predictors do not match xdim");
          m.have_data = true;
        },
        py::arg("successes"), py::arg("trials"), py::arg("predictors"))
      .def_property_readonly("xdim", [](const PyBinomialModel &m) { return m.xdim; })
      .def_property_readonly("coef", py::cpp_function([](PyBinomialModel &m) { return BinomialCoefView{&m}; },
                                                      py::keep_alive<0, 1>()))
      .def_property_readonly("Beta", [](const PyBinomialModel &m) { m.need_impl(); return to_numpy(m.impl->Beta()); })
      .def("set_method", [](PyBinomialModel &m, const Ptr<PosteriorSampler> &s) { m.need_impl(); m.impl->set_method(s); })
      .def("sample_posterior", [](PyBinomialModel &m) { m.need_impl(); m.impl->sample_posterior(); })
      .def("chain_states", [](const PyBinomialModel &m) {
        m.need_impl();
        std::vector<uint8_t> g;
        Vector b;
        m.impl->chain_states(g, b);
        const py::ssize_t p = m.xdim, C = (py::ssize_t)g.size() / p;
        py::array_t<uint8_t> G({C, p});
        py::array_t<double> B({C, p});
        std::memcpy(G.mutable_data(), g.data(), g.size());
        std::memcpy(B.mutable_data(), b.data(), b.size() * 8);
        return py::make_tuple(G, B);
      }, "inclusion indicators and coefficients of EVERY chain");
}

}  // namespace

PYBIND11_MODULE(_boom, boom) {
  boom.doc() = "BayesBoom-shaped bindings of the MI355X spike-and-slab engine (boom_amd)";

  py::class_<PosteriorSampler, Ptr<PosteriorSampler>>(boom, "PosteriorSampler")
      .def("draw", &PosteriorSampler::draw)
      .def("logpri", &PosteriorSampler::logpri)
      .def("set_seed", &PosteriorSampler::set_seed);

  py::class_<MvnGivenScalarSigma, Ptr<MvnGivenScalarSigma>>(boom, "MvnGivenScalarSigma")
      .def(py::init([](const NpArray &mean, const NpArray &unscaled_precision, py::object) {
             return new MvnGivenScalarSigma(vector_from(mean), matrix_from(unscaled_precision));
           }),
           py::arg("mean"), py::arg("unscaled_precision"), py::arg("sigsq") = py::none(),
           "The slab: beta | sigma ~ N(mean, sigma^2 unscaled_precision^{-1}).")
      .def_property_readonly("dim", &MvnGivenScalarSigma::dim);

  py::class_<ChisqModel, Ptr<ChisqModel>>(boom, "ChisqModel")
      .def(py::init<double, double>(), py::arg("df"), py::arg("sigma_estimate"))
      .def_property_readonly("df", &ChisqModel::df)
      .def_property_readonly("sigma", &ChisqModel::sigma);

  py::class_<VariableSelectionPrior, Ptr<VariableSelectionPrior>>(boom, "VariableSelectionPrior")
      .def(py::init([](const NpArray &probs) { return new VariableSelectionPrior(vector_from(probs)); }),
           py::arg("prior_inclusion_probabilities"))
      .def("set_max_model_size", &VariableSelectionPrior::set_max_model_size)
      .def_property_readonly("potential_nvars", &VariableSelectionPrior::potential_nvars);

  py::class_<CoefView>(boom, "GlmCoefs")
      .def("drop_all", [](CoefView &c) { c.model->drop_all(); })
      .def("add", [](CoefView &c, int i) { c.model->add(i); })
      .def("drop", [](CoefView &c, int i) { c.model->drop(i); })
      .def_property_readonly("inc", [](const CoefView &c) {
        const RegressionModel &m = *c.model;
        std::vector<bool> g(m.xdim());
        for (int j = 0; j < m.xdim(); ++j) g[j] = m.inc()[j];
        return g;
      })
      .def_property_readonly("nvars", [](const CoefView &c) {
        const RegressionModel &m = *c.model;
        return m.inc().nvars();
      })
      .def_property_readonly("Beta", [](const CoefView &c) {
        const RegressionModel &m = *c.model;
        return to_numpy(m.Beta());
      });

  py::class_<RegressionModel, Ptr<RegressionModel>>(boom, "RegressionModel")
      .def(py::init([](const NpArray &X, const NpArray &y, bool, int chains, uint64_t seed, int device,
                       const std::vector<int> &devices) {
             if (!devices.empty())
               return new RegressionModel(matrix_from(X), vector_from(y), chains, devices, seed);
             return new RegressionModel(matrix_from(X), vector_from(y), chains, seed, device);
           }),
           py::arg("X"), py::arg("y"), py::arg("start_at_mle") = false, py::arg("chains") = 1,
           py::arg("seed") = 8675309ull, py::arg("device") = 0, py::arg("devices") = std::vector<int>(),
           "RegressionModel(X, y, start_at_mle): sufficient statistics are built on the "
           "device.  chains / seed / device: the many-chain engine behind the model; "
           "devices=[...]: `chains` chains on EACH listed device behind the one model.")
      .def_property_readonly("xdim", &RegressionModel::xdim)
      .def_property_readonly("coef", py::cpp_function([](RegressionModel &m) { return CoefView{&m}; },
                                                      py::keep_alive<0, 1>()))
      .def_property_readonly("Beta", [](const RegressionModel &m) { return to_numpy(m.Beta()); })
      .def_property_readonly("sigsq", &RegressionModel::sigsq)
      .def_property_readonly("sigma", [](const RegressionModel &m) { return std::sqrt(m.sigsq()); })
      .def("set_sigsq", &RegressionModel::set_sigsq)
      .def("set_method", [](RegressionModel &m, const Ptr<PosteriorSampler> &s) { m.set_method(s); })
      .def("clear_methods", &RegressionModel::clear_methods)
      .def("sample_posterior", &RegressionModel::sample_posterior)
      .def("chain_states", [](const RegressionModel &m) {
        std::vector<uint8_t> g;
        Vector b, s;
        m.chain_states(g, b, s);
        const py::ssize_t C = (py::ssize_t)s.size(), p = m.xdim();
        py::array_t<uint8_t> G({C, p});
        py::array_t<double> B({C, p});
        std::memcpy(G.mutable_data(), g.data(), g.size());
        std::memcpy(B.mutable_data(), b.data(), b.size() * 8);
        return py::make_tuple(G, B, to_numpy(s));
      }, "inclusion indicators, coefficients and sigma^2 of EVERY chain");

  py::class_<BregVsSampler, PosteriorSampler, Ptr<BregVsSampler>>(boom, "BregVsSampler")
      .def(py::init([](RegressionModel *model, const Ptr<MvnGivenScalarSigma> &slab,
                       const Ptr<ChisqModel> &residual_precision_prior,
                       const Ptr<VariableSelectionPrior> &spike, py::object) {
             return new BregVsSampler(model, slab, residual_precision_prior, spike);
           }),
           py::arg("model"), py::arg("slab"), py::arg("residual_precision_prior"), py::arg("spike"),
           py::arg("seeding_rng") = py::none(), py::keep_alive<1, 2>(),
           "Create a BregVsSampler -- a spike and slab sampler for regression models.")
      .def("limit_model_selection", [](BregVsSampler &s, int max_flips) { s.limit_model_selection((uint)max_flips); })
      .def("suppress_model_selection", &BregVsSampler::suppress_model_selection)
      .def("set_sigma_upper_limit", &BregVsSampler::set_sigma_upper_limit)
      .def("set_correlation_swap_threshold", &BregVsSampler::set_correlation_swap_threshold)
      .def("set_lookahead", &BregVsSampler::set_lookahead,
           "run n sweeps per launch and hand them out one sample_posterior() at a time");

  // ---- logit / probit spike and slab (GlmModel_def.cpp:549-590, :966-1010) ----------
  py::class_<MvnModel, Ptr<MvnModel>>(boom, "MvnModel")
      .def(py::init([](const NpArray &mu, const NpArray &Sigma, bool ivar) {
             if (!ivar) throw std::runtime_error("MvnModel: pass the precision (ivar=True); the engine works in precisions");
             return new MvnModel(vector_from(mu), matrix_from(Sigma));
           }),
           py::arg("mu"), py::arg("Sigma"), py::arg("ivar") = false,
           "A slab whose precision does not scale with sigma^2 (MvnBase).")
      .def_property_readonly("dim", &MvnModel::dim);

  py::class_<BinomialCoefView>(boom, "BinomialGlmCoefs")
      .def("drop_all", [](BinomialCoefView &c) {
        std::fill(c.model->inc.begin(), c.model->inc.end(), 0);
        if (c.model->impl) c.model->impl->drop_all();
      })
      .def("add", [](BinomialCoefView &c, int i) {
        c.model->inc.at(i) = 1;
        if (c.model->impl) c.model->impl->add(i);
      })
      .def("drop", [](BinomialCoefView &c, int i) {
        c.model->inc.at(i) = 0;
        if (c.model->impl) c.model->impl->drop(i);
      })
      .def_property_readonly("inc", [](const BinomialCoefView &c) {
        std::vector<bool> g(c.model->xdim);
        for (int j = 0; j < c.model->xdim; ++j) g[j] = c.model->impl ? c.model->impl->inc()[j] : c.model->inc[j] != 0;
        return g;
      })
      .def_property_readonly("Beta", [](const BinomialCoefView &c) {
        c.model->need_impl();
        return to_numpy(c.model->impl->Beta());
      });

  struct PyLogit : PyBinomialModel { using PyBinomialModel::PyBinomialModel; };
  struct PyProbit : PyBinomialModel { using PyBinomialModel::PyBinomialModel; };
  py::class_<PyBinomialModel>(boom, "_BinomialRegressionModel");
  py::class_<PyLogit, PyBinomialModel> logit(boom, "BinomialLogitModel");
  logit.def(py::init([](int xdim, bool include_all, int chains, uint64_t seed, int device) {
              return new PyLogit(xdim, include_all, true, chains, seed, device);
            }),
            py::arg("xdim"), py::arg("include_all") = true, py::arg("chains") = 1,
            py::arg("seed") = 8675309ull, py::arg("device") = 0);
  bind_binomial_model(logit);
  py::class_<PyProbit, PyBinomialModel> probit(boom, "BinomialProbitModel");
  probit.def(py::init([](int xdim, bool include_all, int chains, uint64_t seed, int device) {
               return new PyProbit(xdim, include_all, false, chains, seed, device);
             }),
             py::arg("xdim"), py::arg("include_all") = true, py::arg("chains") = 1,
             py::arg("seed") = 8675309ull, py::arg("device") = 0);
  bind_binomial_model(probit);

  py::class_<BinomialLogitSpikeSlabSampler, PosteriorSampler, Ptr<BinomialLogitSpikeSlabSampler>>(
      boom, "BinomialLogitSpikeSlabSampler")
      .def(py::init([](PyLogit &model, const Ptr<MvnModel> &slab, const Ptr<VariableSelectionPrior> &spike,
                       int clt_threshold, py::object) {
             return make_binomial_sampler<BinomialLogitSpikeSlabSampler, BinomialLogitModel>(model, slab, spike,
                                                                                             clt_threshold);
           }),
           py::arg("model"), py::arg("slab"), py::arg("spike"), py::arg("clt_threshold") = 5,
           py::arg("seeding_rng") = py::none(), py::keep_alive<1, 2>())
      .def("limit_model_selection", &BinomialLogitSpikeSlabSampler::limit_model_selection);
  py::class_<BinomialProbitSpikeSlabSampler, PosteriorSampler, Ptr<BinomialProbitSpikeSlabSampler>>(
      boom, "BinomialProbitSpikeSlabSampler")
      .def(py::init([](PyProbit &model, const Ptr<MvnModel> &slab, const Ptr<VariableSelectionPrior> &spike,
                       int clt_threshold, py::object) {
             return make_binomial_sampler<BinomialProbitSpikeSlabSampler, BinomialProbitModel>(model, slab, spike,
                                                                                               clt_threshold);
           }),
           py::arg("model"), py::arg("slab"), py::arg("spike"), py::arg("clt_threshold") = 5,
           py::arg("seeding_rng") = py::none(), py::keep_alive<1, 2>())
      .def("limit_model_selection", &BinomialProbitSpikeSlabSampler::limit_model_selection);

  // ---- bsts: state models, the state-space regression and its sampler
  // (StateModelWrapper.cpp:73-260, StateSpaceModelWrapper.cpp:203-260, :476-490).  The
  // reference attaches one sampler object per variance and one to the observation
  // model; here each state model takes its prior through set_prior and the
  // observation model's three priors go to StateSpacePosteriorSampler.
  py::class_<LocalLevelStateModel, Ptr<LocalLevelStateModel>>(boom, "LocalLevelStateModel")
      .def(py::init<double>(), py::arg("sigma") = 1.0)
      .def("set_initial_state_mean", &LocalLevelStateModel::set_initial_state_mean)
      .def("set_initial_state_variance", &LocalLevelStateModel::set_initial_state_variance)
      .def("set_prior", &LocalLevelStateModel::set_prior, py::arg("df"), py::arg("sigma_guess"),
           py::arg("sigma_upper_limit") = std::numeric_limits<double>::infinity(),
           "ZeroMeanGaussianConjSampler(model, df, sigma_guess) + set_sigma_upper_limit");
  py::class_<LocalLinearTrendStateModel, Ptr<LocalLinearTrendStateModel>>(boom, "LocalLinearTrendStateModel")
      .def(py::init<>())
      .def("set_initial_state_mean", [](LocalLinearTrendStateModel &m, const NpArray &v) { m.set_initial_state_mean(vector_from(v)); })
      .def("set_initial_state_variance", [](LocalLinearTrendStateModel &m, const NpArray &diag) { m.set_initial_state_variance(vector_from(diag)); })
      .def("set_initial_sigma", &LocalLinearTrendStateModel::set_initial_sigma)
      .def("set_prior", &LocalLinearTrendStateModel::set_prior, py::arg("which_variable"), py::arg("df"),
           py::arg("sigma_guess"), py::arg("sigma_upper_limit") = std::numeric_limits<double>::infinity(),
           "ZeroMeanMvnIndependenceSampler(model, df, sigma_guess, which_variable) + set_sigma_upper_limit");
  py::class_<StudentLocalLinearTrendStateModel, Ptr<StudentLocalLinearTrendStateModel>>(boom, "StudentLocalLinearTrendStateModel")
      .def(py::init<double, double, double, double>(), py::arg("sigma_level") = 1.0, py::arg("nu_level") = 1000.0,
           py::arg("sigma_slope") = 1.0, py::arg("nu_slope") = 1000.0)
      .def("set_initial_state_mean", [](StudentLocalLinearTrendStateModel &m, const NpArray &v) { m.set_initial_state_mean(vector_from(v)); })
      .def("set_initial_state_variance", [](StudentLocalLinearTrendStateModel &m, const NpArray &diag) { m.set_initial_state_variance(vector_from(diag)); })
      .def("set_initial_sigma", &StudentLocalLinearTrendStateModel::set_initial_sigma)
      .def("set_initial_nu", &StudentLocalLinearTrendStateModel::set_initial_nu)
      .def("set_prior", &StudentLocalLinearTrendStateModel::set_prior, py::arg("which"), py::arg("df"),
           py::arg("sigma_guess"), py::arg("sigma_upper_limit") = std::numeric_limits<double>::infinity(),
           "which = 0: level, 1: slope; ChisqModel(df, sigma_guess) on sigma^2 + the sigma upper limit")
      .def("set_nu_prior", &StudentLocalLinearTrendStateModel::set_nu_prior, py::arg("which"), py::arg("kind"),
           py::arg("a"), py::arg("b"), "kind 0: uniform(a, b); 1: gamma(a, b)");
  py::class_<SeasonalStateModel, Ptr<SeasonalStateModel>>(boom, "SeasonalStateModel")
      .def(py::init<int, int>(), py::arg("nseasons"), py::arg("season_duration") = 1)
      .def_property_readonly("state_dimension", &SeasonalStateModel::state_dimension)
      .def_property_readonly("nseasons", &SeasonalStateModel::nseasons)
      .def_property_readonly("season_duration", &SeasonalStateModel::season_duration)
      .def("set_time_of_first_observation", &SeasonalStateModel::set_time_of_first_observation)
      .def("set_sigsq", &SeasonalStateModel::set_sigsq)
      .def("set_initial_state_mean", [](SeasonalStateModel &m, const NpArray &v) { m.set_initial_state_mean(vector_from(v)); })
      .def("set_initial_state_variance", &SeasonalStateModel::set_initial_state_variance)
      .def("set_prior", &SeasonalStateModel::set_prior, py::arg("df"), py::arg("sigma_guess"),
           py::arg("sigma_upper_limit") = std::numeric_limits<double>::infinity());

  py::class_<RandomWalkHolidayStateModel, Ptr<RandomWalkHolidayStateModel>>(
      boom, "RandomWalkHolidayStateModel",
      "RandomWalkHolidayStateModel(positions, width).  BayesBoom's constructor takes (holiday, time_zero); this "
      "module has no Date or Holiday classes, so it takes what those two amount to: positions[t] = -1 where "
      "time t is outside the holiday's influence window, else the day's position in the window (0 .. width - 1), "
      "and the window's maximum width.  Entries past the length of the series serve forecasts.")
      .def(py::init([](const std::vector<int32_t> &positions, int width) {
             return new RandomWalkHolidayStateModel(positions, width);
           }),
           py::arg("positions"), py::arg("width"))
      .def_property_readonly("state_dimension", &RandomWalkHolidayStateModel::state_dimension)
      .def_property_readonly("positions", [](const RandomWalkHolidayStateModel &m) { return m.positions(); })
      .def("set_sigsq", &RandomWalkHolidayStateModel::set_sigsq)
      .def("set_initial_state_mean", [](RandomWalkHolidayStateModel &m, const NpArray &v) { m.set_initial_state_mean(vector_from(v)); })
      .def("set_initial_state_variance",
           [](RandomWalkHolidayStateModel &m, const NpArray &v) { m.set_initial_state_variance(vector_from(v)); },
           "the diagonal of the initial state's variance")
      .def("set_prior", &RandomWalkHolidayStateModel::set_prior, py::arg("df"), py::arg("sigma_guess"),
           py::arg("sigma_upper_limit") = std::numeric_limits<double>::infinity());

  py::class_<RegressionHolidayStateModel, Ptr<RegressionHolidayStateModel>>(
      boom, "RegressionHolidayStateModel",
      "RegressionHolidayStateModel(widths, prior_mean, prior_sd): one coefficient per day of each holiday's influence "
      "window, shared across the years, all N(prior_mean, prior_sd^2).  BayesBoom's add_holiday takes a Holiday; this "
      "module has no Date or Holiday classes, so the model takes the holidays' window widths and set_calendar what the "
      "holidays amount to: index[t] = -1 where no holiday of the model is active at time t, else offset_h + the day's "
      "position in holiday h's window (offset_h: the widths of the holidays before h).  Entries past the length of "
      "the series serve forecasts.  The model is no block of the state: state_dimension, state() and "
      "state_variances() of the model that holds it do not count it.")
      .def(py::init([](const std::vector<int32_t> &widths, double prior_mean, double prior_sd) {
             return new RegressionHolidayStateModel(widths, prior_mean, prior_sd);
           }),
           py::arg("widths"), py::arg("prior_mean"), py::arg("prior_sd"))
      .def_property_readonly("number_of_coefficients", &RegressionHolidayStateModel::number_of_coefficients)
      .def_property_readonly("widths", [](const RegressionHolidayStateModel &m) { return m.widths(); })
      .def_property_readonly("calendar", [](const RegressionHolidayStateModel &m) { return m.calendar(); })
      .def("set_calendar", &RegressionHolidayStateModel::set_calendar, py::arg("index"))
      .def("set_coefficients", [](RegressionHolidayStateModel &m, const NpArray &v) { m.set_coefficients(vector_from(v)); },
           py::arg("coefficients"), "the initial coefficients, one per day of every holiday's window (default: zeros)");

  py::class_<HierarchicalRegressionHolidayStateModel, Ptr<HierarchicalRegressionHolidayStateModel>>(
      boom, "HierarchicalRegressionHolidayStateModel",
      "HierarchicalRegressionHolidayStateModel(nholidays, width, mean_prior_mean, mean_prior_variance, variance_guess, "
      "variance_guess_weight): nholidays holidays of one window width whose coefficient vectors are N(mu, Omega^-1), with "
      "mu ~ N(mean_prior_mean, mean_prior_variance) and Omega ~ Wishart(variance_guess_weight, variance_guess_weight x "
      "variance_guess) drawn by HierGaussianRegressionAsisSampler.  As RegressionHolidayStateModel it takes a calendar in "
      "place of Holiday objects: index[t] = -1, or h x width + the day's position in holiday h's window.")
      .def(py::init([](int nholidays, int width, const NpArray &mean, const NpArray &variance, const NpArray &guess, double weight) {
             return new HierarchicalRegressionHolidayStateModel(nholidays, width, vector_from(mean), matrix_from(variance),
                                                                matrix_from(guess), weight);
           }),
           py::arg("nholidays"), py::arg("width"), py::arg("mean_prior_mean"), py::arg("mean_prior_variance"),
           py::arg("variance_guess"), py::arg("variance_guess_weight"))
      .def_property_readonly("number_of_coefficients", &HierarchicalRegressionHolidayStateModel::number_of_coefficients)
      .def_property_readonly("calendar", [](const HierarchicalRegressionHolidayStateModel &m) { return m.calendar(); })
      .def("set_calendar", &HierarchicalRegressionHolidayStateModel::set_calendar, py::arg("index"))
      .def("set_coefficients", [](HierarchicalRegressionHolidayStateModel &m, const NpArray &v) { m.set_coefficients(vector_from(v)); },
           py::arg("coefficients"), "the initial coefficients, holiday by holiday (default: zeros)")
      .def("holiday_mean", [](const HierarchicalRegressionHolidayStateModel &m, int chain) { return to_numpy(m.holiday_mean(chain)); },
           py::arg("chain") = 0, "mu in one chain's draw")
      .def("holiday_precision", [](const HierarchicalRegressionHolidayStateModel &m, int chain) { return matrix_to_numpy(m.holiday_precision(chain)); },
           py::arg("chain") = 0, "Omega in one chain's draw");

  py::class_<DynamicRegressionStateModel, Ptr<DynamicRegressionStateModel>>(
      boom, "DynamicRegressionStateModel",
      "DynamicRegressionStateModel(predictors): regression coefficients that follow independent random walks.  "
      "predictors: rows x d, row t = x_t; rows past the length of the series serve forecasts.  One variance, "
      "ChisqModel(df, sigma_guess) prior and sigma upper limit per coefficient.")
      .def(py::init([](const NpArray &predictors) { return new DynamicRegressionStateModel(matrix_from(predictors)); }),
           py::arg("predictors"))
      .def_property_readonly("state_dimension", &DynamicRegressionStateModel::state_dimension)
      .def_property_readonly("xdim", &DynamicRegressionStateModel::xdim)
      .def_property_readonly("predictors", [](const DynamicRegressionStateModel &m) {
        py::array_t<double> out({m.rows(), m.xdim()});
        std::copy(m.predictors().begin(), m.predictors().end(), out.mutable_data());
        return out;
      })
      .def("set_sigsq", [](DynamicRegressionStateModel &m, const NpArray &v) { m.set_sigsq(vector_from(v)); },
           "the coefficients' innovation variances")
      .def("set_initial_state_mean", [](DynamicRegressionStateModel &m, const NpArray &v) { m.set_initial_state_mean(vector_from(v)); })
      .def("set_initial_state_variance",
           [](DynamicRegressionStateModel &m, const NpArray &v) { m.set_initial_state_variance(vector_from(v)); },
           "the diagonal of the initial state's variance")
      .def("set_prior", &DynamicRegressionStateModel::set_prior, py::arg("coefficient"), py::arg("df"), py::arg("sigma_guess"),
           py::arg("sigma_upper_limit") = std::numeric_limits<double>::infinity());

  py::class_<DynamicRegressionArStateModel, Ptr<DynamicRegressionArStateModel>>(
      boom, "DynamicRegressionArStateModel",
      "DynamicRegressionArStateModel(predictors, lags): regression coefficients that each follow an autoregression "
      "of `lags` lags.  predictors: rows x d, row t = x_t; rows past the length of the series serve forecasts.  "
      "Per coefficient one ArModel (phi, sigma) with a ChisqModel(df, sigma_guess) prior and sigma upper limit.  "
      "The arrays over the state (initial mean and variance, phi) are d x lags.")
      .def(py::init([](const NpArray &predictors, int lags) { return new DynamicRegressionArStateModel(matrix_from(predictors), lags); }),
           py::arg("predictors"), py::arg("lags"))
      .def_property_readonly("state_dimension", &DynamicRegressionArStateModel::state_dimension)
      .def_property_readonly("xdim", &DynamicRegressionArStateModel::xdim)
      .def_property_readonly("lags", &DynamicRegressionArStateModel::lags)
      .def_property_readonly("predictors", [](const DynamicRegressionArStateModel &m) {
        py::array_t<double> out({m.rows(), m.xdim()});
        std::copy(m.predictors().begin(), m.predictors().end(), out.mutable_data());
        return out;
      })
      .def("set_sigsq", [](DynamicRegressionArStateModel &m, const NpArray &v) { m.set_sigsq(vector_from(v)); },
           "the coefficients' innovation variances")
      .def("set_phi", [](DynamicRegressionArStateModel &m, const NpArray &v) { m.set_phi(vector_from(v)); },
           "the autoregressions' initial coefficients, d x lags (row-major), every row stationary")
      .def("set_initial_state_mean", [](DynamicRegressionArStateModel &m, const NpArray &v) { m.set_initial_state_mean(vector_from(v)); })
      .def("set_initial_state_variance",
           [](DynamicRegressionArStateModel &m, const NpArray &v) { m.set_initial_state_variance(vector_from(v)); },
           "the diagonal of the initial state's variance")
      .def("set_prior", &DynamicRegressionArStateModel::set_prior, py::arg("coefficient"), py::arg("df"), py::arg("sigma_guess"),
           py::arg("sigma_upper_limit") = std::numeric_limits<double>::infinity());

  py::class_<MonthlyAnnualCycle, Ptr<MonthlyAnnualCycle>>(
      boom, "MonthlyAnnualCycle",
      "MonthlyAnnualCycle(year, month, day): a month-of-year effect for daily data, 12 seasons that start on the "
      "first day of a month.  BayesBoom's constructor takes a Date; this module has no Date class, so it takes the "
      "date of the first observation as three integers.  set_forecast_horizon: the steps past the series that the "
      "block's calendar covers (366 by default).")
      .def(py::init<int, int, int>(), py::arg("year"), py::arg("month"), py::arg("day"))
      .def_property_readonly("state_dimension", &MonthlyAnnualCycle::state_dimension)
      .def_property_readonly("nseasons", &MonthlyAnnualCycle::nseasons)
      .def("set_forecast_horizon", &MonthlyAnnualCycle::set_forecast_horizon, py::arg("steps"))
      .def("calendar", [](const MonthlyAnnualCycle &m, int length) {
             const std::vector<uint8_t> f = m.calendar(length);
             return std::vector<int>(f.begin(), f.end());
           }, py::arg("length"), "the season-start flags of a series of `length` time points and the horizon beyond it")
      .def("set_sigsq", &MonthlyAnnualCycle::set_sigsq)
      .def("set_initial_state_mean", [](MonthlyAnnualCycle &m, const NpArray &v) { m.set_initial_state_mean(vector_from(v)); })
      .def("set_initial_state_variance", &MonthlyAnnualCycle::set_initial_state_variance)
      .def("set_prior", &MonthlyAnnualCycle::set_prior, py::arg("df"), py::arg("sigma_guess"),
           py::arg("sigma_upper_limit") = std::numeric_limits<double>::infinity());

  py::class_<ArStateModel, Ptr<ArStateModel>>(boom, "ArStateModel")
      .def(py::init<int>(), py::arg("number_of_lags"))
      .def_property_readonly("state_dimension", &ArStateModel::state_dimension)
      .def_property_readonly("number_of_lags", &ArStateModel::number_of_lags)
      .def("set_phi", [](ArStateModel &m, const NpArray &v) { m.set_phi(vector_from(v)); })
      .def("set_sigma", &ArStateModel::set_sigma)
      .def("set_sigsq", &ArStateModel::set_sigsq)
      .def("set_initial_state_mean", [](ArStateModel &m, const NpArray &v) { m.set_initial_state_mean(vector_from(v)); })
      .def("set_initial_state_variance", &ArStateModel::set_initial_state_variance)
      .def("set_spike_slab_prior",
           [](ArStateModel &m, const NpArray &mu, const NpArray &siginv, const NpArray &pi, double df, double sigma_guess,
              double sigma_upper_limit, bool truncate, int max_flips) {
             m.set_spike_slab_prior(vector_from(mu), matrix_from(siginv), vector_from(pi), df, sigma_guess,
                                    sigma_upper_limit, truncate, max_flips);
           },
           py::arg("mu"), py::arg("siginv"), py::arg("pi"), py::arg("df"), py::arg("sigma_guess"),
           py::arg("sigma_upper_limit") = std::numeric_limits<double>::infinity(), py::arg("truncate") = true,
           py::arg("max_flips") = -1,
           "bsts AddAutoAr: ArSpikeSlabSampler(model, MvnModel(mu, siginv), VariableSelectionPrior(pi), "
           "ChisqModel(df, sigma_guess), truncate) in place of the ArPosteriorSampler")
      .def("set_prior", &ArStateModel::set_prior, py::arg("df"), py::arg("sigma_guess"),
           py::arg("sigma_upper_limit") = std::numeric_limits<double>::infinity(),
           "ArPosteriorSampler(model, ChisqModel(df, sigma_guess)) + set_sigma_upper_limit");

  py::class_<StaticInterceptStateModel, Ptr<StaticInterceptStateModel>>(boom, "StaticInterceptStateModel")
      .def(py::init<>())
      .def_property_readonly("state_dimension", &StaticInterceptStateModel::state_dimension)
      .def("set_initial_state_mean", &StaticInterceptStateModel::set_initial_state_mean)
      .def("set_initial_state_variance", &StaticInterceptStateModel::set_initial_state_variance);

  py::class_<TrigStateModel, Ptr<TrigStateModel>>(boom, "TrigStateModel")
      .def(py::init([](double period, const NpArray &frequencies) {
             return new TrigStateModel(period, vector_from(frequencies));
           }),
           py::arg("period"), py::arg("frequencies"))
      .def_property_readonly("state_dimension", &TrigStateModel::state_dimension)
      .def("set_sigsq", &TrigStateModel::set_sigsq)
      .def("set_initial_state_mean", [](TrigStateModel &m, const NpArray &v) { m.set_initial_state_mean(vector_from(v)); })
      .def("set_initial_state_variance",
           [](TrigStateModel &m, const NpArray &v) { m.set_initial_state_variance(vector_from(v)); },
           "the diagonal of the initial state's variance")
      .def("set_prior", &TrigStateModel::set_prior, py::arg("df"), py::arg("sigma_guess"),
           py::arg("sigma_upper_limit") = std::numeric_limits<double>::infinity(),
           "ZeroMeanGaussianConjSampler(error_distribution(), ChisqModel(df, sigma_guess)) + set_sigma_upper_limit");

  py::class_<ZeroMeanGaussianModel, Ptr<ZeroMeanGaussianModel>>(boom, "ZeroMeanGaussianModel")
      .def(py::init<double>(), py::arg("sigma") = 1.0)
      .def_property_readonly("sigma", &ZeroMeanGaussianModel::sigma);
  py::class_<NonzeroMeanAr1Model, Ptr<NonzeroMeanAr1Model>>(boom, "NonzeroMeanAr1Model")
      .def(py::init<double, double, double>(), py::arg("mu") = 0.0, py::arg("phi") = 0.0, py::arg("sigma") = 1.0)
      .def_property_readonly("mu", &NonzeroMeanAr1Model::mu)
      .def_property_readonly("phi", &NonzeroMeanAr1Model::phi)
      .def_property_readonly("sigma", &NonzeroMeanAr1Model::sigma);
  py::class_<SemilocalLinearTrendStateModel, Ptr<SemilocalLinearTrendStateModel>>(boom, "SemilocalLinearTrendStateModel")
      .def(py::init<const Ptr<ZeroMeanGaussianModel> &, const Ptr<NonzeroMeanAr1Model> &>(), py::arg("level"),
           py::arg("slope"))
      .def_property_readonly("state_dimension", &SemilocalLinearTrendStateModel::state_dimension)
      .def("set_initial_level_mean", &SemilocalLinearTrendStateModel::set_initial_level_mean)
      .def("set_initial_level_sd", &SemilocalLinearTrendStateModel::set_initial_level_sd)
      .def("set_initial_slope_mean", &SemilocalLinearTrendStateModel::set_initial_slope_mean)
      .def("set_initial_slope_sd", &SemilocalLinearTrendStateModel::set_initial_slope_sd)
      .def("set_level_prior", &SemilocalLinearTrendStateModel::set_level_prior, py::arg("df"), py::arg("sigma_guess"),
           py::arg("sigma_upper_limit") = std::numeric_limits<double>::infinity(),
           "ZeroMeanGaussianConjSampler(level, df, sigma_guess) + set_sigma_upper_limit")
      .def("set_slope_prior", &SemilocalLinearTrendStateModel::set_slope_prior, py::arg("mean_mu"),
           py::arg("mean_sigma"), py::arg("ar1_mu"), py::arg("ar1_sigma"), py::arg("df"), py::arg("sigma_guess"),
           py::arg("sigma_upper_limit") = std::numeric_limits<double>::infinity(), py::arg("force_stationary") = true,
           py::arg("force_ar1_positive") = false,
           "NonzeroMeanAr1Sampler(slope, mean prior, AR(1) coefficient prior, ChisqModel(df, sigma_guess)) + its switches");

  py::class_<StateSpaceRegressionModel, Ptr<StateSpaceRegressionModel>>(boom, "StateSpaceRegressionModel")
      .def(py::init([](const NpArray &response, const NpArray &predictors, const std::vector<bool> &is_observed,
                       int chains, uint64_t seed, int device) {
             return new StateSpaceRegressionModel(vector_from(response), matrix_from(predictors), is_observed,
                                                  chains, seed, device);
           }),
           py::arg("response"), py::arg("predictors"), py::arg("is_observed") = std::vector<bool>(),
           py::arg("chains") = 1, py::arg("seed") = 8675309ull, py::arg("device") = 0)
      .def_property_readonly("xdim", &StateSpaceRegressionModel::xdim)
      .def_property_readonly("time_dimension", &StateSpaceRegressionModel::time_dimension)
      .def_property_readonly("state_dimension", &StateSpaceRegressionModel::state_dimension)
      .def("one_step_prediction_errors", [](StateSpaceRegressionModel &m, bool standardize) {
             return matrix_to_numpy(m.one_step_prediction_errors(standardize));
           }, py::arg("standardize") = false,
           "the one-step prediction errors of every chain's current draw (time_dimension x chains)")
      .def("one_step_holdout_prediction_errors", [](StateSpaceRegressionModel &m, const NpArray &newX, const NpArray &newY, bool standardize) {
             return matrix_to_numpy(m.one_step_holdout_prediction_errors(matrix_from(newX), vector_from(newY), standardize));
           }, py::arg("newX"), py::arg("newY"), py::arg("standardize") = false,
           "the one-step prediction errors of the holdout rows behind the series, from every chain's current draw and final state (chains x horizon)")
      .def("log_likelihood", [](StateSpaceRegressionModel &m) { return to_numpy(m.log_likelihood()); },
           "the filter's log likelihood of every chain's current draw (one entry per chain)")
      .def("add_state", [](StateSpaceRegressionModel &m, const Ptr<LocalLevelStateModel> &s) { m.add_state(s); })
      .def("add_state", [](StateSpaceRegressionModel &m, const Ptr<LocalLinearTrendStateModel> &s) { m.add_state(s); })
      .def("add_state", [](StateSpaceRegressionModel &m, const Ptr<SeasonalStateModel> &s) { m.add_state(s); })
      .def("add_state", [](StateSpaceRegressionModel &m, const Ptr<ArStateModel> &s) { m.add_state(s); })
      .def("add_state", [](StateSpaceRegressionModel &m, const Ptr<StaticInterceptStateModel> &s) { m.add_state(s); })
      .def("add_state", [](StateSpaceRegressionModel &m, const Ptr<TrigStateModel> &s) { m.add_state(s); })
      .def("add_state", [](StateSpaceRegressionModel &m, const Ptr<SemilocalLinearTrendStateModel> &s) { m.add_state(s); })
      .def("add_state", [](StateSpaceRegressionModel &m, const Ptr<StudentLocalLinearTrendStateModel> &s) { m.add_state(s); })
      .def("add_state", [](StateSpaceRegressionModel &m, const Ptr<RandomWalkHolidayStateModel> &s) { m.add_state(s); })
      .def("add_state", [](StateSpaceRegressionModel &m, const Ptr<DynamicRegressionStateModel> &s) { m.add_state(s); })
      .def("add_state", [](StateSpaceRegressionModel &m, const Ptr<DynamicRegressionArStateModel> &s) { m.add_state(s); })
      .def("add_state", [](StateSpaceRegressionModel &m, const Ptr<RegressionHolidayStateModel> &s) { m.add_state(s); })
      .def("add_state", [](StateSpaceRegressionModel &m, const Ptr<HierarchicalRegressionHolidayStateModel> &s) { m.add_state(s); })
      .def("regression_holiday_coefficients", [](const StateSpaceRegressionModel &m, int chain, int which) {
             return to_numpy(m.regression_holiday_coefficients(chain, which));
           }, py::arg("chain") = 0, py::arg("which") = 0,
           "the coefficients of the which-th RegressionHolidayStateModel in one chain's draw")
      .def("add_state", [](StateSpaceRegressionModel &m, const Ptr<MonthlyAnnualCycle> &s) { m.add_state(s); })
      .def("student_trend_nu", [](const StateSpaceRegressionModel &m, int chain) { return to_numpy(m.student_trend_nu(chain)); },
           py::arg("chain") = 0, "(nu_level, nu_slope) of the StudentLocalLinearTrendStateModel in one chain's draw")
      .def("student_trend_weights", [](const StateSpaceRegressionModel &m, int chain) {
        const Matrix w = m.student_trend_weights(chain);
        py::array_t<double> out({(py::ssize_t)w.nrow(), (py::ssize_t)w.ncol()});
        auto o = out.mutable_unchecked<2>();
        for (int i = 0; i < w.nrow(); ++i)
          for (int j = 0; j < w.ncol(); ++j) o(i, j) = w(i, j);
        return out;
      }, py::arg("chain") = 0, "the StudentLocalLinearTrendStateModel's weights in one chain: (2, T), level then slope")
      .def("semilocal_slope", [](const StateSpaceRegressionModel &m, int chain, int which) { return to_numpy(m.semilocal_slope(chain, which)); },
           py::arg("chain") = 0, py::arg("which") = 0,
           "(AR(1) coefficient, long-run mean) of the which-th SemilocalLinearTrendStateModel's slope in one chain's draw")
      .def_property_readonly("number_of_state_models", &StateSpaceRegressionModel::number_of_state_models)
      .def("dynamic_regression_ar_phi",
           [](const StateSpaceRegressionModel &m, int chain, int which) { return matrix_to_numpy(m.dynamic_regression_ar_phi(chain, which)); },
           py::arg("chain") = 0, py::arg("which") = 0,
           "the autoregression coefficients of the which-th DynamicRegressionArStateModel in one chain's current draw, d x lags")
      .def("ar_phi", [](const StateSpaceRegressionModel &m, int chain, int which) { return to_numpy(m.ar_phi(chain, which)); },
           py::arg("chain") = 0, py::arg("which") = 0,
           "the coefficients of the which-th ArStateModel in one chain's current draw")
      .def("ar_sigsq", &StateSpaceRegressionModel::ar_sigsq, py::arg("chain") = 0, py::arg("which") = 0)
      .def("ar_inclusion", [](const StateSpaceRegressionModel &m, int chain, int which) {
             const std::vector<bool> g = m.ar_inclusion(chain, which);
             py::array_t<bool> out((py::ssize_t)g.size());
             auto o = out.mutable_unchecked<1>();
             for (size_t i = 0; i < g.size(); ++i) o(i) = g[i];
             return out;
           }, py::arg("chain") = 0, py::arg("which") = 0,
           "the inclusion indicators of the which-th ArStateModel (ArSpikeSlabSampler: set_spike_slab_prior) in one chain's current draw")
      .def("set_method", [](StateSpaceRegressionModel &m, const Ptr<PosteriorSampler> &s) { m.set_method(s); })
      .def("sample_posterior", &StateSpaceRegressionModel::sample_posterior)
      .def("state", [](const StateSpaceRegressionModel &m, int chain) {
        if (!m.structural()) return py::array(to_numpy(m.state(chain)));
        const Matrix st = m.structural_state(chain);
        py::array_t<double> out({(py::ssize_t)st.nrow(), (py::ssize_t)st.ncol()});
        auto w = out.mutable_unchecked<2>();
        for (int i = 0; i < st.nrow(); ++i)
          for (int j = 0; j < st.ncol(); ++j) w(i, j) = st(i, j);
        return py::array(out);
      }, py::arg("chain") = 0, "the state draw of one chain: (T,) for the local level, (state_dimension, T) otherwise")
      .def("state_variances", [](const StateSpaceRegressionModel &m, int chain) {
        if (!m.structural()) { Vector v(1, m.level_sigsq(chain)); return to_numpy(v); }
        return to_numpy(m.state_variances(chain));
      }, py::arg("chain") = 0, "every variance parameter in state-model order (a local linear trend has two)")
      .def("chain_states", [](const StateSpaceRegressionModel &m) {
        const py::ssize_t C = m.engine()->chains(), p = m.xdim();
        py::array_t<uint8_t> G({C, p});
        py::array_t<double> B({C, p}), S((py::ssize_t)C);
        m.engine()->check(ba_get_states(m.engine()->get(), G.mutable_data(), B.mutable_data(), S.mutable_data()));
        return py::make_tuple(G, B, S);
      }, "inclusion indicators, coefficients and residual variances of EVERY chain");

  py::class_<StateSpacePosteriorSampler, PosteriorSampler, Ptr<StateSpacePosteriorSampler>>(
      boom, "StateSpacePosteriorSampler")
      .def(py::init([](StateSpaceRegressionModel *model, const Ptr<MvnGivenScalarSigma> &slab,
                       const Ptr<ChisqModel> &residual_precision_prior, const Ptr<VariableSelectionPrior> &spike,
                       double sigma_upper_limit, py::object) {
             return new StateSpacePosteriorSampler(model, slab, residual_precision_prior, spike, sigma_upper_limit);
           }),
           py::arg("model"), py::arg("slab"), py::arg("residual_precision_prior"), py::arg("spike"),
           py::arg("sigma_upper_limit") = std::numeric_limits<double>::infinity(),
           py::arg("seeding_rng") = py::none(), py::keep_alive<1, 2>())
      .def("set_lookahead", &StateSpacePosteriorSampler::set_lookahead,
           "enqueue n sweep rounds at a time and hand them out one sample_posterior() at a time (default 64)");

  // ---- Poisson regression spike and slab (GlmModel_def.cpp: PoissonRegressionModel,
  // PoissonRegressionSpikeSlabSampler) ---------------------------------------------------
  py::class_<PoissonRegressionModel, Ptr<PoissonRegressionModel>>(boom, "PoissonRegressionModel")
      .def(py::init([](const NpArray &X, const NpArray &y, const NpArray &exposure, int chains, uint64_t seed,
                       int device) {
             return new PoissonRegressionModel(matrix_from(X), vector_from(y), vector_from(exposure), chains, seed,
                                               device);
           }),
           py::arg("predictors"), py::arg("response"), py::arg("exposure"), py::arg("chains") = 1,
           py::arg("seed") = 8675309ull, py::arg("device") = 0)
      .def_property_readonly("xdim", &PoissonRegressionModel::xdim)
      .def("set_mixture_table", [](PoissonRegressionModel &m, const std::vector<int64_t> &counts,
                                   const std::vector<int32_t> &ncomp, const NpArray &mu, const NpArray &sigma,
                                   const NpArray &weight, int64_t largest_index) {
             NormalMixtureTable t;
             t.counts = counts; t.ncomp = ncomp;
             t.mu = vector_from(mu); t.sigma = vector_from(sigma); t.weight = vector_from(weight);
             t.largest_index = largest_index;
             m.set_mixture_table(t);
           },
           py::arg("counts"), py::arg("ncomp"), py::arg("mu"), py::arg("sigma"), py::arg("weight"),
           py::arg("largest_index"),
           "the reference's normal mixtures for the negative log-gamma densities (its data)")
      .def("drop_all", &PoissonRegressionModel::drop_all)
      .def("add", &PoissonRegressionModel::add)
      .def("drop", &PoissonRegressionModel::drop)
      .def_property_readonly("inc", [](const PoissonRegressionModel &m) {
        std::vector<bool> g(m.xdim());
        for (int j = 0; j < m.xdim(); ++j) g[j] = m.inc()[j];
        return g;
      })
      .def_property_readonly("Beta", [](const PoissonRegressionModel &m) { return to_numpy(m.Beta()); })
      .def("set_Beta", [](PoissonRegressionModel &m, const NpArray &b) { m.set_Beta(vector_from(b)); })
      .def("set_method", [](PoissonRegressionModel &m, const Ptr<PosteriorSampler> &s) { m.set_method(s); })
      .def("sample_posterior", &PoissonRegressionModel::sample_posterior)
      .def("chain_states", [](const PoissonRegressionModel &m) {
        const py::ssize_t C = m.engine()->chains(), p = m.xdim();
        py::array_t<uint8_t> G({C, p});
        py::array_t<double> B({C, p});
        m.engine()->check(ba_get_states(m.engine()->get(), G.mutable_data(), B.mutable_data(), nullptr));
        return py::make_tuple(G, B);
      }, "inclusion indicators and coefficients of EVERY chain");
  py::class_<PoissonRegressionSpikeSlabSampler, PosteriorSampler, Ptr<PoissonRegressionSpikeSlabSampler>>(
      boom, "PoissonRegressionSpikeSlabSampler")
      .def(py::init([](PoissonRegressionModel *model, const Ptr<MvnModel> &slab,
                       const Ptr<VariableSelectionPrior> &spike, int, py::object) {
             return new PoissonRegressionSpikeSlabSampler(model, slab, spike);
           }),
           py::arg("model"), py::arg("slab"), py::arg("spike"), py::arg("number_of_threads") = 1,
           py::arg("seeding_rng") = py::none(), py::keep_alive<1, 2>())
      .def("limit_model_selection", &PoissonRegressionSpikeSlabSampler::limit_model_selection);

  // ---- Student-t regression spike and slab (GlmModel_def.cpp:468-495) ----------------------
  py::class_<DoubleModel, Ptr<DoubleModel>>(boom, "DoubleModel");
  py::class_<UniformModel, DoubleModel, Ptr<UniformModel>>(boom, "UniformModel")
      .def(py::init<double, double>(), py::arg("lo") = 0.0, py::arg("hi") = 1.0)
      .def_property_readonly("lo", &UniformModel::lo)
      .def_property_readonly("hi", &UniformModel::hi);
  py::class_<GammaModel, DoubleModel, Ptr<GammaModel>>(boom, "GammaModel")
      .def(py::init<double, double>(), py::arg("a") = 1.0, py::arg("b") = 1.0, "shape a, rate b")
      .def_property_readonly("alpha", &GammaModel::alpha)
      .def_property_readonly("beta", &GammaModel::beta);
  py::class_<TRegressionModel, Ptr<TRegressionModel>>(boom, "TRegressionModel")
      .def(py::init([](const NpArray &X, const NpArray &y, int chains, uint64_t seed, int device) {
             return new TRegressionModel(matrix_from(X), vector_from(y), chains, seed, device);
           }),
           py::arg("predictors"), py::arg("response"), py::arg("chains") = 1,
           py::arg("seed") = 8675309ull, py::arg("device") = 0)
      .def("drop_all", &TRegressionModel::drop_all)
      .def("add", &TRegressionModel::add)
      .def("drop", &TRegressionModel::drop)
      .def_property_readonly("inc", [](const TRegressionModel &m) {
        std::vector<bool> g(m.xdim());
        for (int j = 0; j < m.xdim(); ++j) g[j] = m.inc()[j];
        return g;
      })
      .def_property_readonly("Beta", [](const TRegressionModel &m) { return to_numpy(m.Beta()); })
      .def("set_Beta", [](TRegressionModel &m, const NpArray &b) { m.set_Beta(vector_from(b)); })
      .def_property_readonly("sigsq", &TRegressionModel::sigsq)
      .def_property_readonly("sigma", [](const TRegressionModel &m) { return std::sqrt(m.sigsq()); })
      .def_property_readonly("nu", &TRegressionModel::nu)
      .def("set_sigsq", &TRegressionModel::set_sigsq)
      .def("set_nu", &TRegressionModel::set_nu)
      .def("set_method", [](TRegressionModel &m, const Ptr<PosteriorSampler> &s) { m.set_method(s); })
      .def("sample_posterior", &TRegressionModel::sample_posterior);
  py::class_<TRegressionSpikeSlabSampler, PosteriorSampler, Ptr<TRegressionSpikeSlabSampler>>(
      boom, "TRegressionSpikeSlabSampler")
      .def(py::init([](TRegressionModel *model, const Ptr<MvnGivenScalarSigma> &slab,
                       const Ptr<VariableSelectionPrior> &spike, const Ptr<ChisqModel> &siginv_prior,
                       const Ptr<DoubleModel> &nu_prior, py::object) {
             return new TRegressionSpikeSlabSampler(model, slab, spike, siginv_prior, nu_prior);
           }),
           py::arg("model"), py::arg("coefficient_slab"), py::arg("coefficient_spike"),
           py::arg("siginv_prior"), py::arg("nu_prior"), py::arg("seeding_rng") = py::none(),
           py::keep_alive<1, 2>())
      .def("draw", &TRegressionSpikeSlabSampler::draw)
      .def("set_sigma_upper_limit", &TRegressionSpikeSlabSampler::set_sigma_upper_limit)
      .def("limit_model_selection", &TRegressionSpikeSlabSampler::limit_model_selection)
      .def("allow_model_selection", &TRegressionSpikeSlabSampler::allow_model_selection);

  // ---- bsts family = "student" (StateSpaceStudentRegressionModel,
  // StateSpaceStudentPosteriorSampler): the state space model's bindings, inherited, + the
  // Student-t observation model's ----------------------------------------------------------
  py::class_<StateSpaceStudentRegressionModel, StateSpaceRegressionModel, Ptr<StateSpaceStudentRegressionModel>>(
      boom, "StateSpaceStudentRegressionModel")
      .def(py::init([](const NpArray &response, const NpArray &predictors, const std::vector<bool> &is_observed,
                       int chains, uint64_t seed, int device) {
             return new StateSpaceStudentRegressionModel(vector_from(response), matrix_from(predictors), is_observed,
                                                         chains, seed, device);
           }),
           py::arg("response"), py::arg("predictors"), py::arg("is_observed") = std::vector<bool>(),
           py::arg("chains") = 1, py::arg("seed") = 8675309ull, py::arg("device") = 0)
      .def("nu", &StateSpaceStudentRegressionModel::nu, py::arg("chain") = 0)
      .def("set_nu", &StateSpaceStudentRegressionModel::set_nu)
      .def("sigsq", &StateSpaceStudentRegressionModel::sigsq, py::arg("chain") = 0)
      .def("weights", [](const StateSpaceStudentRegressionModel &m, int chain) { return to_numpy(m.weights(chain)); },
           py::arg("chain") = 0, "the latent gamma weights of one chain (0 at a missing step)")
      .def("set_weights", [](StateSpaceStudentRegressionModel &m, const NpArray &w, int chain) {
             m.set_weights(vector_from(w), chain);
           }, py::arg("weights"), py::arg("chain") = -1)
      .def("impute_state", &StateSpaceStudentRegressionModel::impute_state)
      .def("simulate_forecast", [](StateSpaceStudentRegressionModel &m, const NpArray &predictors) {
             return forecast_to_numpy(m.simulate_forecast(matrix_from(predictors)));
           }, py::arg("predictors"), "one predictive draw of the next observations per chain (chains x horizon)");
  py::class_<StateSpaceStudentPosteriorSampler, PosteriorSampler, Ptr<StateSpaceStudentPosteriorSampler>>(
      boom, "StateSpaceStudentPosteriorSampler")
      .def(py::init([](StateSpaceStudentRegressionModel *model, const Ptr<MvnGivenScalarSigma> &slab,
                       const Ptr<VariableSelectionPrior> &spike, const Ptr<ChisqModel> &siginv_prior,
                       const Ptr<DoubleModel> &nu_prior, py::object) {
             return new StateSpaceStudentPosteriorSampler(model, slab, spike, siginv_prior, nu_prior);
           }),
           py::arg("model"), py::arg("coefficient_slab"), py::arg("coefficient_spike"),
           py::arg("siginv_prior"), py::arg("nu_prior"), py::arg("seeding_rng") = py::none(),
           py::keep_alive<1, 2>())
      .def("draw", &StateSpaceStudentPosteriorSampler::draw)
      .def("set_sigma_upper_limit", &StateSpaceStudentPosteriorSampler::set_sigma_upper_limit);

  // ---- bsts family = "poisson" (StateSpacePoissonModel, StateSpacePoissonPosteriorSampler): the
  // state space model's bindings, inherited, + the Poisson observation model's ------------------
  latent_data_class(py::class_<StateSpacePoissonModel, StateSpaceRegressionModel, Ptr<StateSpacePoissonModel>>(
                        boom, "StateSpacePoissonModel"), "exposure",
                    "one predictive draw of the next counts per chain (chains x horizon); exposure: default ones")
      .def(py::init([](const NpArray &counts, const NpArray &exposure, const NpArray &predictors,
                       const std::vector<bool> &is_observed, int chains, uint64_t seed, int device) {
             return new StateSpacePoissonModel(vector_from(counts), vector_from(exposure), matrix_from(predictors),
                                               is_observed, chains, seed, device);
           }),
           py::arg("counts"), py::arg("exposure"), py::arg("predictors"), py::arg("is_observed") = std::vector<bool>(),
           py::arg("chains") = 1, py::arg("seed") = 8675309ull, py::arg("device") = 0)
      .def("set_mixture_table", [](StateSpacePoissonModel &m, const std::vector<int64_t> &counts,
                                   const std::vector<int32_t> &ncomp, const NpArray &mu, const NpArray &sigma,
                                   const NpArray &weight, int64_t largest_index) {
             NormalMixtureTable t;
             t.counts = counts; t.ncomp = ncomp;
             t.mu = vector_from(mu); t.sigma = vector_from(sigma); t.weight = vector_from(weight);
             t.largest_index = largest_index;
             m.set_mixture_table(t);
           },
           py::arg("counts"), py::arg("ncomp"), py::arg("mu"), py::arg("sigma"), py::arg("weight"),
           py::arg("largest_index"),
           "the reference's normal mixtures for the negative log-gamma densities (its data)");
  py::class_<StateSpacePoissonPosteriorSampler, PosteriorSampler, Ptr<StateSpacePoissonPosteriorSampler>>(
      boom, "StateSpacePoissonPosteriorSampler")
      .def(py::init([](StateSpacePoissonModel *model, const Ptr<MvnModel> &slab,
                       const Ptr<VariableSelectionPrior> &spike, py::object) {
             return new StateSpacePoissonPosteriorSampler(model, slab, spike);
           }),
           py::arg("model"), py::arg("slab"), py::arg("spike"), py::arg("seeding_rng") = py::none(),
           py::keep_alive<1, 2>())
      .def("draw", &StateSpacePoissonPosteriorSampler::draw)
      .def("limit_model_selection", &StateSpacePoissonPosteriorSampler::limit_model_selection);

  // ---- bsts family = "logit" (StateSpaceLogitModel, StateSpaceLogitPosteriorSampler): the state
  // space model's bindings, inherited, + the binomial logit observation model's -----------------
  latent_data_class(py::class_<StateSpaceLogitModel, StateSpaceRegressionModel, Ptr<StateSpaceLogitModel>>(
                        boom, "StateSpaceLogitModel"), "trials",
                    "one predictive draw of the next success counts per chain (chains x horizon); trials: default ones")
      .def(py::init([](const NpArray &successes, const NpArray &trials, const NpArray &predictors,
                       const std::vector<bool> &is_observed, int chains, uint64_t seed, int device, int clt_threshold) {
             return new StateSpaceLogitModel(vector_from(successes), vector_from(trials), matrix_from(predictors),
                                             is_observed, chains, seed, device, clt_threshold);
           }),
           py::arg("successes"), py::arg("trials"), py::arg("predictors"), py::arg("is_observed") = std::vector<bool>(),
           py::arg("chains") = 1, py::arg("seed") = 8675309ull, py::arg("device") = 0, py::arg("clt_threshold") = 5);
  py::class_<StateSpaceLogitPosteriorSampler, PosteriorSampler, Ptr<StateSpaceLogitPosteriorSampler>>(
      boom, "StateSpaceLogitPosteriorSampler")
      .def(py::init([](StateSpaceLogitModel *model, const Ptr<MvnModel> &slab,
                       const Ptr<VariableSelectionPrior> &spike, py::object) {
             return new StateSpaceLogitPosteriorSampler(model, slab, spike);
           }),
           py::arg("model"), py::arg("slab"), py::arg("spike"), py::arg("seeding_rng") = py::none(),
           py::keep_alive<1, 2>())
      .def("draw", &StateSpaceLogitPosteriorSampler::draw)
      .def("limit_model_selection", &StateSpaceLogitPosteriorSampler::limit_model_selection);

  // ---- quantile regression spike and slab (QuantileRegressionModel,
  // QuantileRegressionSpikeSlabSampler) -----------------------------------------------------
  py::class_<QuantileRegressionModel, Ptr<QuantileRegressionModel>>(boom, "QuantileRegressionModel")
      .def(py::init<int, double, int, uint64_t, int>(), py::arg("xdim"), py::arg("quantile"),
           py::arg("chains") = 1, py::arg("seed") = 8675309ull, py::arg("device") = 0)
      .def_property_readonly("xdim", &QuantileRegressionModel::xdim)
      .def_property_readonly("quantile", &QuantileRegressionModel::quantile)
      .def("set_data", [](QuantileRegressionModel &m, const NpArray &X, const NpArray &y) {
             m.set_data(matrix_from(X), vector_from(y));
           },
           py::arg("predictors"), py::arg("response"))
      .def("drop_all", &QuantileRegressionModel::drop_all)
      .def("add", &QuantileRegressionModel::add)
      .def("drop", &QuantileRegressionModel::drop)
      .def_property_readonly("inc", [](const QuantileRegressionModel &m) {
        std::vector<bool> g(m.xdim());
        for (int j = 0; j < m.xdim(); ++j) g[j] = m.inc()[j];
        return g;
      })
      .def_property_readonly("Beta", [](const QuantileRegressionModel &m) { return to_numpy(m.Beta()); })
      .def("set_Beta", [](QuantileRegressionModel &m, const NpArray &b) { m.set_Beta(vector_from(b)); })
      .def("set_method", [](QuantileRegressionModel &m, const Ptr<PosteriorSampler> &s) { m.set_method(s); })
      .def("sample_posterior", &QuantileRegressionModel::sample_posterior);
  py::class_<QuantileRegressionSpikeSlabSampler, PosteriorSampler, Ptr<QuantileRegressionSpikeSlabSampler>>(
      boom, "QuantileRegressionSpikeSlabSampler")
      .def(py::init([](QuantileRegressionModel *model, const Ptr<MvnModel> &slab,
                       const Ptr<VariableSelectionPrior> &spike, py::object) {
             return new QuantileRegressionSpikeSlabSampler(model, slab, spike);
           }),
           py::arg("model"), py::arg("slab"), py::arg("spike"), py::arg("seeding_rng") = py::none(),
           py::keep_alive<1, 2>())
      .def("draw", &QuantileRegressionSpikeSlabSampler::draw)
      .def("limit_model_selection", &QuantileRegressionSpikeSlabSampler::limit_model_selection);
  // ---- multinomial logit spike and slab (MultinomialLogitModel, MLVS: the names of the
  // reference's Models/Glm) ----------------------------------------------------------------
  boom.def("mlvs_flip_order", [](int n) { return mlvs_flip_order(n); }, py::arg("n"),
           "the order MLVS::draw_inclusion_vector visits n coefficients in: the shuffle of 0 .. n - 1 "
           "by a freshly constructed std::default_random_engine");
  py::class_<MultinomialLogitModel, Ptr<MultinomialLogitModel>>(boom, "MultinomialLogitModel")
      .def(py::init<int, int, int, int, uint64_t, int>(), py::arg("nchoices"), py::arg("subject_xdim"),
           py::arg("choice_xdim"), py::arg("chains") = 1, py::arg("seed") = 8675309ull, py::arg("device") = 0)
      .def_property_readonly("Nchoices", &MultinomialLogitModel::Nchoices)
      .def_property_readonly("subject_nvars", &MultinomialLogitModel::subject_nvars)
      .def_property_readonly("choice_nvars", &MultinomialLogitModel::choice_nvars)
      .def_property_readonly("beta_size", &MultinomialLogitModel::beta_size)
      .def("set_data", [](MultinomialLogitModel &m, const std::vector<int32_t> &y, py::object Xs, py::object Xc) {
             const Matrix xs = Xs.is_none() ? Matrix() : matrix_from(Xs.cast<NpArray>());
             const Matrix xc = Xc.is_none() ? Matrix() : matrix_from(Xc.cast<NpArray>());
             m.set_data(y, xs, xc);
           },
           py::arg("response"), py::arg("subject_predictors"), py::arg("choice_predictors"))
      .def("drop_all", &MultinomialLogitModel::drop_all)
      .def("add", &MultinomialLogitModel::add)
      .def("drop", &MultinomialLogitModel::drop)
      .def_property_readonly("inc", [](const MultinomialLogitModel &m) {
        std::vector<bool> g(m.beta_size());
        for (int j = 0; j < m.beta_size(); ++j) g[j] = m.coef().inc()[j];
        return g;
      })
      .def_property_readonly("beta", [](const MultinomialLogitModel &m) { return to_numpy(m.beta()); })
      .def("set_beta", [](MultinomialLogitModel &m, const NpArray &b) { m.set_beta(vector_from(b)); })
      .def("set_method", [](MultinomialLogitModel &m, const Ptr<PosteriorSampler> &s) { m.set_method(s); })
      .def("sample_posterior", &MultinomialLogitModel::sample_posterior);
  py::class_<MLVS, PosteriorSampler, Ptr<MLVS>>(boom, "MLVS")
      .def(py::init([](MultinomialLogitModel *model, const Ptr<MvnModel> &slab,
                       const Ptr<VariableSelectionPrior> &spike, py::object) {
             return new MLVS(model, slab, spike);
           }),
           py::arg("model"), py::arg("slab"), py::arg("spike"), py::arg("seeding_rng") = py::none(),
           py::keep_alive<1, 2>())
      .def("draw", &MLVS::draw)
      .def("suppress_model_selection", &MLVS::suppress_model_selection)
      .def("allow_model_selection", &MLVS::allow_model_selection)
      .def("limit_model_selection", &MLVS::limit_model_selection)
      .def("max_nflips", &MLVS::max_nflips)
      .def("logpri", &MLVS::logpri);
}
