// GroundRemoval / GroundRemoval2 / RangeImage through the C++ mirror (include/smhip/filters.h): the classes configured from XML
// text, the opt-in Factory on text holding a commented-out filter, and the default Factory unchanged.  Prints a JSON verdict.
#include <cmath>
#include <cstdio>
#include <random>

#include "smhip/filters.h"

using namespace smhip::pre_processers::filter;
using smhip::data::InnerCloudType;
using smhip::data::InnerPointType;

static int g_fail = 0;
#define CHECK_T(c) do { if (!(c)) { ++g_fail; std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); } } while (0)

// a flat ground at -1.73 m around the sensor; every third point anywhere from -1 m to 2 m
static InnerCloudType::Ptr Scene(unsigned seed) {
  std::mt19937 gen(seed);
  std::uniform_real_distribution<float> az(0.f, 6.2831853f), rg(2.f, 60.f), h(-1.0f, 2.0f), noise(-0.01f, 0.01f);
  InnerCloudType::Ptr c(new InnerCloudType);
  c->stamp = 7;
  for (int i = 0; i < 30000; ++i) {
    InnerPointType p;
    const float a = az(gen), r = rg(gen);
    p.x = r * std::cos(a); p.y = r * std::sin(a);
    p.z = (i % 3 == 0) ? h(gen) : -1.73f + noise(gen);
    p.intensity = 0.5f;
    c->points.push_back(p);
  }
  return c;
}

static const char* kXml =
    "<filters>\n"
    "  <filter name=\"Range\" ><param type=\"1\" name=\"min_range\"> 5. </param></filter>\n"
    "  <!-- <filter name=\"GroundRemoval2\" >\n"
    "    <param type=\"1\" name=\"r_min\"> 0.1 </param>\n"
    "  </filter> -->\n"
    "  <filter name=\"GroundRemoval2\" >\n"
    "    <param type=\"1\" name=\"r_min\"> 0.1 </param>\n"
    "    <param type=\"1\" name=\"start_ground_height\"> -1.5 </param>\n"
    "    <param type=\"1\" name=\"long_line_threshold\"> 10 </param>\n"
    "    <param type=\"1\" name=\"max_slope\"> 0.12 </param>\n"
    "    <param type=\"1\" name=\"max_error\"> 0.1 </param>\n"
    "    <param type=\"1\" name=\"max_dist_to_line\"> 0.10 </param>\n"
    "    <param type=\"1\" name=\"max_start_height\"> 0.6 </param>\n"
    "    <param type=\"0\" name=\"thread_num\"> 4 </param>\n"
    "  </filter>\n"
    "  <filter name=\"RangeImage\" >\n"
    "    <param type=\"1\" name=\"btm_angle\"> -20. </param>\n"
    "    <param type=\"0\" name=\"vertical_line_num\"> 60 </param>\n"
    "  </filter>\n"
    "</filters>\n";

int main() {
  auto raw = Scene(3);
  const size_t n = raw->points.size();
  {  // the three classes from XML text
    GroundRemoval2 g;
    CHECK_T(g.InitFromXmlText("<filter name=\"GroundRemoval2\" ><param type=\"1\" name=\"start_ground_height\"> -1.7 </param>"
                              "<param type=\"0\" name=\"bin_num\"> 150 </param><param type=\"0\" name=\"thread_num\"> 4 </param></filter>"));
    CHECK_T(g.DescEx().i[0] == 150 && g.DescEx().i[1] == 180 && g.DescEx().p[2] == -1.7f);
    g.SetInputCloud(raw);
    InnerCloudType::Ptr out(new InnerCloudType);
    g.Filter(out);
    CHECK_T(out->stamp == raw->stamp);
    CHECK_T(out->points.size() + g.Outliers().size() == n && g.Inliers().size() == out->points.size());
    CHECK_T(g.Outliers().size() > n / 8);                                  // many ground points go (about a third of them)
    for (int i : g.Outliers()) CHECK_T(raw->points[i].z < -1.5f);        // and nothing high
    CHECK_T(!g.InitFromXmlText("<filter name=\"GroundRemoval2\" ><param type=\"0\" name=\"segment_num\"> 0 </param></filter>"));

    GroundRemoval gr;
    CHECK_T(gr.InitFromXmlText("<filter name=\"GroundRemoval\" ><param type=\"1\" name=\"leaf_size\"> 0.5 </param>"
                               "<param type=\"0\" name=\"min_point_num_in_voxel\"> 2 </param></filter>"));
    CHECK_T(gr.DescEx().p[0] == 0.5f && gr.DescEx().i[0] == 2);
    gr.SetInputCloud(raw);
    gr.Filter(out);
    CHECK_T(!out->points.empty() && out->points.size() < n);
    for (size_t k = 1; k < gr.Inliers().size(); ++k) CHECK_T(gr.Inliers()[k - 1] < gr.Inliers()[k]);   // input order

    RangeImage ri;
    CHECK_T(ri.InitFromXmlText("<filter name=\"RangeImage\" ><param type=\"0\" name=\"vertical_line_num\"> 60 </param></filter>"));
    CHECK_T(ri.DescEx().i[0] == 60 && ri.DescEx().i[1] == 1800);
    ri.SetInputCloud(raw);
    ri.Filter(out);
    CHECK_T(!out->points.empty() && out->points.size() <= 60u * 1800u);
  }
  {  // opt-in factory: the commented-out filter is skipped, the real ones are read
    Factory fac(true);
    fac.InitFromXmlText(kXml);
    CHECK_T(fac.size() == 3);
    fac.SetInputCloud(raw);
    InnerCloudType::Ptr out(new InnerCloudType);
    fac.Filter(out);
    CHECK_T(!out->points.empty() && out->points.size() < n);
    int m = 0;
    CHECK_T(fac.FilterToSource(DeviceContext::Default()->handle(), 0, &m) && m == static_cast<int>(out->points.size()));
    Factory later;
    later.EnableGroundFilters();
    later.InitFromXmlText(kXml);
    CHECK_T(later.size() == 3);
    auto copy = std::static_pointer_cast<Factory>(fac.CreateNewInstance());
    copy->InitFromXmlText(kXml);
    CHECK_T(copy->size() == 3);
  }
  {  // the default factory keeps its set and its parse
    Factory fac;
    fac.InitFromXmlText(kXml);
    CHECK_T(fac.size() == 1);                                              // Range only: the ground filters are not registered
  }
  std::printf("{\"failed\": %d}\n", g_fail);
  return g_fail ? 1 : 0;
}
