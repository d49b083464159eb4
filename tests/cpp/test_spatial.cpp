// test_spatial.cpp -- include/cilantro_hip/spatial.hpp: the parts that need no device (the empty polytope, polytopes given by halfspaces,
// containsPoint, transform, the calls that are not built); with "device" also a hull and a region query on the GPU.
#include <cilantro_hip/spatial.hpp>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

using namespace cilantro_hip;

static const std::vector<float> kCube = {1, 0, 0, -1, -1, 0, 0, 0, 0, 1, 0, -1, 0, -1, 0, 0, 0, 0, 1, -1, 0, 0, -1, 0};      // six halfspaces of [0, 1]^3

template <class Fn> static bool throws(Fn&& fn) { try { fn(); } catch (const std::runtime_error&) { return true; } return false; }

int main(int argc, char** argv) {
  ConvexPolytope3f empty;
  CHECK(empty.isEmpty() && empty.getVertices().empty() && empty.getArea() == 0.0 && empty.getVolume() == 0.0);
  CHECK(empty.getFacetHyperplanes() == std::vector<float>({1, 0, 0, 1, -1, 0, 0, 1}));
  CHECK(std::isnan(empty.getInteriorPoint()[0]));
  const float origin[3] = {0, 0, 0}, mid[3] = {0.5f, 0.5f, 0.5f}, face[3] = {1.0f, 0.5f, 0.5f}, out[3] = {1.5f, 0.5f, 0.5f};
  CHECK(!empty.containsPoint(origin));
  ConvexPolytope2f empty2;
  CHECK(empty2.isEmpty() && empty2.getFacetHyperplanes() == std::vector<float>({1, 0, 1, -1, 0, 1}));

  ConvexPolytope3f cube = ConvexPolytope3f::fromHalfspaces(kCube);
  CHECK(!cube.isEmpty() && cube.numFacets() == 6);
  CHECK(cube.containsPoint(mid) && cube.containsPoint(face) && !cube.containsPoint(out) && !cube.containsPoint(face, 0.01f) && cube.containsPoint(out, -0.6f));
  CHECK(throws([&] { cube.getVertices(); }) && throws([&] { cube.intersectionWith(cube); }));

  const float R[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1}, t[3] = {10, 20, 30};      // a quarter turn about z, then a shift
  ConvexPolytope3f moved = cube.transformed(R, t);
  const float mid_moved[3] = {-0.5f + 10, 0.5f + 20, 0.5f + 30}, out_moved[3] = {-0.5f + 10, 1.5f + 20, 0.5f + 30};
  CHECK(moved.containsPoint(mid_moved) && !moved.containsPoint(out_moved) && !moved.containsPoint(mid));
  const float T[16] = {0, -1, 0, 10, 1, 0, 0, 20, 0, 0, 1, 30, 0, 0, 0, 1};
  CHECK(cube.transformed(T).getFacetHyperplanes() == moved.getFacetHyperplanes());

  SpaceRegion3f region = SpaceRegion3f(cube).unionWith(SpaceRegion3f(moved));
  CHECK(region.getConvexPolytopes().size() == 2 && !region.isEmpty());
  CHECK(region.containsPoint(mid) && region.containsPoint(mid_moved) && !region.containsPoint(out));
  CHECK(SpaceRegion3f(empty).isEmpty() && std::isnan(SpaceRegion3f(empty).getInteriorPoint()[0]));
  CHECK(throws([&] { region.complement(); }) && throws([&] { region.getVolume(); }) && throws([&] { region.intersectionWith(region); }) && throws([&] { region.relativeComplement(region); }));
  std::printf("host OK\n");

  if (argc > 1 && std::strcmp(argv[1], "device") == 0) {
    const std::vector<float> pts = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 1, 1, 1, 0, 1, 1, 1, 0, 1, 1, 1, 0.5f, 0.5f, 0.5f};
    ConvexHull3f hull(pts, true);
    CHECK(hull.getVertices().size() == 24 && hull.getFacetVertexIndices().size() == 6 && std::fabs(hull.getVolume() - 1.0) < 1e-12 && std::fabs(hull.getArea() - 6.0) < 1e-12);
    const std::vector<float> q = {0.5f, 0.5f, 0.5f, 1.5f, 0.5f, 0.5f, 1.0f, 1.0f, 1.0f};
    const std::vector<bool> m = SpaceRegion3f(hull).getInteriorPointsIndexMask(q.data(), 3);
    CHECK(m[0] && !m[1] && m[2]);
    CHECK(hull.getInteriorPointIndices(q.data(), 3) == std::vector<size_t>({0, 2}));
    FlatConvexHull3f flat(std::vector<float>({0, 0, 1, 2, 0, 1, 2, 1, 1, 0, 1, 1, 1, 0.5f, 1}).data(), 5);
    CHECK(!flat.isEmpty() && flat.getVertices3D().size() == 12 && std::fabs(flat.getVolume() - 2.0) < 1e-5);
    std::printf("device OK\n");
  }
  return 0;
}
