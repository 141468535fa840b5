// Host-side self-test of the GBDT launchers whose signatures grew for missing_policy="learn"
// (gbdt.hip launch_gbdt_bin / launch_gbdt_split / launch_gbdt_predict, quantile.hip
// launch_quantile_select), for monotone constraints (launch_gbdt_split / launch_gbdt_leaf) and for
// interaction constraints (launch_gbdt_split) and for reg_alpha / max_delta_step (launch_gbdt_split /
// launch_gbdt_leaf): every argument check must throw BEFORE anything is
// launched, whatever the new trailing arguments are, and the old call forms (trailing arguments
// left out) must still compile.  Built with -fsanitize=address,undefined on the host side (tools/sanitize_host.sh); it
// needs no GPU: a call that passes its checks either launches or reports the missing device as a
// std::runtime_error from check_launch, and both count as "got past the checks".
#include <cstdint>
#include <cstdio>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "launchers.h"

namespace {

int failures = 0;

template <typename F>
void expect_refused(const char* what, const char* needle, F&& f) {
  try {
    f();
  } catch (const std::exception& e) {
    if (std::string(e.what()).find(needle) != std::string::npos) return;
    std::printf("FAIL %s: refused with an unexpected message: %s\n", what, e.what());
    ++failures;
    return;
  }
  std::printf("FAIL %s: not refused\n", what);
  ++failures;
}

// Past the checks: a launch, or the runtime's own error where there is no device.
template <typename F>
void expect_checked(const char* what, F&& f) {
  try {
    f();
  } catch (const std::runtime_error& e) {
    if (std::string(e.what()).find("fdx kernel launch failed") != std::string::npos ||
        std::string(e.what()).find("memset failed") != std::string::npos)
      return;
    std::printf("FAIL %s: refused a valid call: %s\n", what, e.what());
    ++failures;
  }
}

}  // namespace

int main() {
  int ndev = 0;
  const bool have_gpu = hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
  // host buffers stand in for device memory: with a GPU present nothing valid is launched on them
  std::vector<float> f32(64 * 32, 0.0f);
  std::vector<int> i32(256, 1);
  std::vector<uint8_t> u8(64 * 32, 0);
  std::vector<long long> i64(256, 0);
  std::vector<int64_t> gc(256, 0);
  std::vector<double> f64(256, 0.0);
  std::vector<unsigned long long> hist(16, 0);
  const int64_t counts[32] = {0};

  for (bool missing : {false, true}) {
    expect_refused("gbdt_bin d = 31", "at most 30 features", [&] {
      fdx::launch_gbdt_bin(f32.data(), 1, 31, 31, f32.data(), i32.data(), u8.data(), nullptr, missing);
    });
    expect_refused("gbdt_split level = -1", "level out of range", [&] {
      fdx::launch_gbdt_split(hist.data(), gc.data(), -1, 4, i32.data(), f32.data(), 1.0, 1.0, 1.0, 1.0, 0.0, i32.data(),
                             i32.data(), f32.data(), f64.data(), i64.data(), i64.data(), nullptr, nullptr, missing);
    });
    expect_refused("gbdt_split level = 8", "level out of range", [&] {
      fdx::launch_gbdt_split(hist.data(), gc.data(), 8, 4, i32.data(), f32.data(), 1.0, 1.0, 1.0, 1.0, 0.0, i32.data(),
                             i32.data(), f32.data(), f64.data(), i64.data(), i64.data(), nullptr, nullptr, missing);
    });
    for (int d : {0, 31})
      expect_refused("gbdt_split bad d", "bad feature count", [&] {
        fdx::launch_gbdt_split(hist.data(), gc.data(), 0, d, i32.data(), f32.data(), 1.0, 1.0, 1.0, 1.0, 0.0,
                               i32.data(), i32.data(), f32.data(), f64.data(), i64.data(), i64.data(), nullptr, nullptr,
                               missing);
      });
  }
  // monotone constraints (launch_gbdt_split / launch_gbdt_leaf trailing arguments): the masks are
  // checked against each other, against d and against the bounds pointers before any launch
  for (bool missing : {false, true}) {
    auto split = [&](int d, uint32_t inc, uint32_t dec, double* lo, double* hi) {
      fdx::launch_gbdt_split(hist.data(), gc.data(), 0, d, i32.data(), f32.data(), 1.0, 1.0, 1.0, 1.0, 0.0, i32.data(),
                             i32.data(), f32.data(), f64.data(), i64.data(), i64.data(), nullptr, nullptr, missing, inc,
                             dec, lo, hi);
    };
    expect_refused("gbdt_split overlapping masks", "monotone masks overlap",
                   [&] { split(4, 0x3u, 0x2u, f64.data(), f64.data()); });
    expect_refused("gbdt_split inc bit = d", "mask bit at or above d", [&] { split(4, 0x10u, 0x1u, f64.data(), f64.data()); });
    expect_refused("gbdt_split dec bit 31", "mask bit at or above d",
                   [&] { split(30, 0x1u, 0x80000000u, f64.data(), f64.data()); });
    expect_refused("gbdt_split masks, no bounds", "need both bounds arrays", [&] { split(4, 0x1u, 0x2u, nullptr, nullptr); });
    expect_refused("gbdt_split masks, lo only", "need both bounds arrays", [&] { split(4, 0x1u, 0x0u, f64.data(), nullptr); });
    expect_refused("gbdt_split masks, hi only", "need both bounds arrays", [&] { split(4, 0x0u, 0x2u, nullptr, f64.data()); });
    // the earlier checks still come first, whatever the masks are
    expect_refused("gbdt_split bad d with masks", "bad feature count", [&] { split(31, 0x1u, 0x1u, nullptr, nullptr); });
  }
  // interaction constraints (launch_gbdt_split's last two arguments): the group masks are host
  // values, checked against their number, against d and against the path pointer before any launch,
  // with and without the monotone tail
  std::vector<uint32_t> pathw(256, 0u);
  for (bool missing : {false, true})
    for (uint32_t inc : {0x0u, 0x1u}) {
      auto split = [&](int d, const std::vector<uint32_t>& groups, uint32_t* path) {
        fdx::launch_gbdt_split(hist.data(), gc.data(), 0, d, i32.data(), f32.data(), 1.0, 1.0, 1.0, 1.0, 0.0,
                               i32.data(), i32.data(), f32.data(), f64.data(), i64.data(), i64.data(), nullptr, nullptr,
                               missing, inc, 0u, f64.data(), f64.data(), groups, path);
      };
      expect_refused("gbdt_split 33 groups", "at most 32 interaction groups",
                     [&] { split(4, std::vector<uint32_t>(33, 0x1u), pathw.data()); });
      expect_refused("gbdt_split group bit = d", "interaction group bit at or above d",
                     [&] { split(4, {0x3u, 0x10u}, pathw.data()); });
      expect_refused("gbdt_split group bit 31", "interaction group bit at or above d",
                     [&] { split(30, {0x80000000u}, pathw.data()); });
      expect_refused("gbdt_split empty group", "empty interaction group", [&] { split(4, {0x3u, 0x0u}, pathw.data()); });
      expect_refused("gbdt_split groups, no path", "need the path array", [&] { split(4, {0x3u}, nullptr); });
      expect_refused("gbdt_split path, no groups", "needs interaction groups", [&] { split(4, {}, pathw.data()); });
      // the earlier checks still come first, whatever the groups are
      expect_refused("gbdt_split bad d with groups", "bad feature count", [&] { split(31, {0x3u}, nullptr); });
    }
  // reg_alpha / max_delta_step (the last two arguments of launch_gbdt_split and launch_gbdt_leaf):
  // host values, finite and >= 0, checked before any launch with every other tail there or not
  {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    for (bool missing : {false, true})
      for (uint32_t inc : {0x0u, 0x1u})
        for (bool groups : {false, true}) {
          auto split = [&](int d, double alpha, double mds) {
            fdx::launch_gbdt_split(hist.data(), gc.data(), 0, d, i32.data(), f32.data(), 1.0, 1.0, 1.0, 1.0, 0.0,
                                   i32.data(), i32.data(), f32.data(), f64.data(), i64.data(), i64.data(), nullptr,
                                   nullptr, missing, inc, 0u, f64.data(), f64.data(),
                                   groups ? std::vector<uint32_t>{0x3u} : std::vector<uint32_t>{},
                                   groups ? pathw.data() : nullptr, alpha, mds);
          };
          expect_refused("gbdt_split alpha < 0", "reg_alpha must be finite and >= 0", [&] { split(4, -1.0, 0.0); });
          expect_refused("gbdt_split alpha NaN", "reg_alpha must be finite and >= 0", [&] { split(4, nan, 1.0); });
          expect_refused("gbdt_split alpha inf", "reg_alpha must be finite and >= 0", [&] { split(4, inf, 0.0); });
          expect_refused("gbdt_split mds < 0", "max_delta_step must be finite and >= 0", [&] { split(4, 0.0, -0.5); });
          expect_refused("gbdt_split mds NaN", "max_delta_step must be finite and >= 0", [&] { split(4, 1.0, nan); });
          expect_refused("gbdt_split mds inf", "max_delta_step must be finite and >= 0", [&] { split(4, 0.0, inf); });
          // the earlier checks still come first, whatever the two values are
          expect_refused("gbdt_split bad d with alpha", "bad feature count", [&] { split(31, -1.0, nan); });
        }
    for (double* b : {static_cast<double*>(nullptr), f64.data()}) {
      auto leaf = [&](double alpha, double mds) {
        fdx::launch_gbdt_leaf(i64.data(), i64.data(), 3, 1.0, 1.0, 1.0, 1.0, 0.1, f32.data(), nullptr, b, b, alpha, mds);
      };
      expect_refused("gbdt_leaf alpha < 0", "reg_alpha must be finite and >= 0", [&] { leaf(-1.0, 0.0); });
      expect_refused("gbdt_leaf alpha NaN", "reg_alpha must be finite and >= 0", [&] { leaf(nan, 0.0); });
      expect_refused("gbdt_leaf alpha inf", "reg_alpha must be finite and >= 0", [&] { leaf(inf, 0.0); });
      expect_refused("gbdt_leaf mds < 0", "max_delta_step must be finite and >= 0", [&] { leaf(0.0, -1.0); });
      expect_refused("gbdt_leaf mds NaN", "max_delta_step must be finite and >= 0", [&] { leaf(0.0, nan); });
      expect_refused("gbdt_leaf mds inf", "max_delta_step must be finite and >= 0", [&] { leaf(1.0, inf); });
    }
    expect_refused("gbdt_leaf lo only with alpha", "both arrays or neither", [&] {
      fdx::launch_gbdt_leaf(i64.data(), i64.data(), 3, 1.0, 1.0, 1.0, 1.0, 0.1, f32.data(), nullptr, f64.data(), nullptr,
                            -1.0, 0.0);
    });
  }
  expect_refused("gbdt_leaf lo only", "both arrays or neither", [&] {
    fdx::launch_gbdt_leaf(i64.data(), i64.data(), 3, 1.0, 1.0, 1.0, 1.0, 0.1, f32.data(), nullptr, f64.data(), nullptr);
  });
  expect_refused("gbdt_leaf hi only", "both arrays or neither", [&] {
    fdx::launch_gbdt_leaf(i64.data(), i64.data(), 3, 1.0, 1.0, 1.0, 1.0, 0.1, f32.data(), nullptr, nullptr, f64.data());
  });
  for (const uint8_t* dleft : {static_cast<const uint8_t*>(nullptr), static_cast<const uint8_t*>(u8.data())}) {
    for (int depth : {0, 9})
      expect_refused("gbdt_predict bad depth", "depth must be in [1, 8]", [&] {
        fdx::launch_gbdt_predict(f32.data(), 1, 30, 30, i32.data(), f32.data(), f32.data(), 1, depth, 0.0f, f32.data(),
                                 nullptr, dleft);
      });
    expect_refused("gbdt_predict d = 31", "at most 30 features", [&] {
      fdx::launch_gbdt_predict(f32.data(), 1, 31, 31, i32.data(), f32.data(), f32.data(), 1, 3, 0.0f, f32.data(), nullptr,
                               dleft);
    });
    // no rows: returns before any launch, with or without the bytes
    fdx::launch_gbdt_predict(f32.data(), 0, 30, 30, i32.data(), f32.data(), f32.data(), 1, 3, 0.0f, f32.data(), nullptr,
                             dleft);
  }
  for (const int64_t* c : {static_cast<const int64_t*>(nullptr), counts}) {
    expect_refused("quantile_select d = 0", "quantile_select: need", [&] {
      fdx::launch_quantile_select(f32.data(), 8, 1, 4, 0, 16, f32.data(), f32.data(), nullptr, c);
    });
    expect_refused("quantile_select d = 33", "quantile_select: need", [&] {
      fdx::launch_quantile_select(f32.data(), 8, 1, 33, 33, 16, f32.data(), f32.data(), nullptr, c);
    });
    expect_refused("quantile_select max_bin = 1", "quantile_select: need", [&] {
      fdx::launch_quantile_select(f32.data(), 8, 1, 4, 4, 1, f32.data(), f32.data(), nullptr, c);
    });
    expect_refused("quantile_select max_bin = 257", "quantile_select: need", [&] {
      fdx::launch_quantile_select(f32.data(), 8, 1, 4, 4, 257, f32.data(), f32.data(), nullptr, c);
    });
    expect_refused("quantile_select m = 0", "quantile_select: need", [&] {
      fdx::launch_quantile_select(f32.data(), 0, 1, 4, 4, 16, f32.data(), f32.data(), nullptr, c);
    });
    expect_refused("quantile_select m = 2^31", "at most 2^31 - 1", [&] {
      fdx::launch_quantile_select(f32.data(), (int64_t)1 << 31, 1, 4, 4, 16, f32.data(), f32.data(), nullptr, c);
    });
  }
  // the call forms from before the trailing arguments existed still compile, and reach the same checks
  expect_refused("gbdt_bin, old form", "at most 30 features", [&] {
    fdx::launch_gbdt_bin(f32.data(), 1, 31, 31, f32.data(), i32.data(), u8.data(), nullptr);
  });
  expect_refused("gbdt_split, old form", "level out of range", [&] {
    fdx::launch_gbdt_split(hist.data(), gc.data(), -1, 4, i32.data(), f32.data(), 1.0, 1.0, 1.0, 1.0, 0.0, i32.data(),
                           i32.data(), f32.data(), f64.data(), i64.data(), i64.data(), nullptr);
  });
  // ... and the forms that end at the monotone and at the interaction arguments
  expect_refused("gbdt_split, monotone form", "level out of range", [&] {
    fdx::launch_gbdt_split(hist.data(), gc.data(), -1, 4, i32.data(), f32.data(), 1.0, 1.0, 1.0, 1.0, 0.0, i32.data(),
                           i32.data(), f32.data(), f64.data(), i64.data(), i64.data(), nullptr, nullptr, false, 0x1u, 0u,
                           f64.data(), f64.data());
  });
  expect_refused("gbdt_split, interaction form", "level out of range", [&] {
    fdx::launch_gbdt_split(hist.data(), gc.data(), -1, 4, i32.data(), f32.data(), 1.0, 1.0, 1.0, 1.0, 0.0, i32.data(),
                           i32.data(), f32.data(), f64.data(), i64.data(), i64.data(), nullptr, nullptr, false, 0u, 0u,
                           nullptr, nullptr, {0x3u}, pathw.data());
  });
  expect_refused("gbdt_predict, old form", "depth must be in [1, 8]", [&] {
    fdx::launch_gbdt_predict(f32.data(), 1, 30, 30, i32.data(), f32.data(), f32.data(), 1, 0, 0.0f, f32.data(), nullptr);
  });
  expect_refused("quantile_select, old form", "quantile_select: need", [&] {
    fdx::launch_quantile_select(f32.data(), 0, 1, 4, 4, 16, f32.data(), f32.data(), nullptr);
  });
  if (!have_gpu) {  // valid arguments without a device: past the checks, then the runtime's error
    for (bool missing : {false, true})
      expect_checked("gbdt_bin, valid", [&] {
        fdx::launch_gbdt_bin(f32.data(), 4, 32, 30, f32.data(), i32.data(), u8.data(), nullptr, missing);
      });
    // disjoint masks below d with both bounds, and the leaf's old call form: past the checks
    expect_checked("gbdt_leaf, old form", [&] {
      fdx::launch_gbdt_leaf(i64.data(), i64.data(), 3, 1.0, 1.0, 1.0, 1.0, 0.1, f32.data(), nullptr);
    });
    // the monotone form and valid reg_alpha / max_delta_step (zero included): past the checks
    expect_checked("gbdt_leaf, monotone form", [&] {
      fdx::launch_gbdt_leaf(i64.data(), i64.data(), 3, 1.0, 1.0, 1.0, 1.0, 0.1, f32.data(), nullptr, f64.data(),
                            f64.data());
    });
    for (double alpha : {0.0, 0.5})
      for (double mds : {0.0, 2.0})
        expect_checked("gbdt_leaf, valid alpha / mds", [&] {
          fdx::launch_gbdt_leaf(i64.data(), i64.data(), 3, 1.0, 1.0, 1.0, 1.0, 0.1, f32.data(), nullptr, nullptr, nullptr,
                                alpha, mds);
        });
  }
  if (failures) {
    std::printf("gbdt_args_selftest: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("gbdt_args_selftest: ok (%s)\n", have_gpu ? "GPU present: argument checks only" : "no GPU");
  return 0;
}
