// StatisticRemoval through the C++ mirror (include/smhip/filters.h), host side only: the class and the opt-in Factory configured
// from XML text, the default Factory unchanged, an unknown parameter refused.  Needs libsmhip.so for the defaults and
// ConfigsValid(), and no GPU: nothing here filters a cloud.  Prints a JSON verdict; `unknown` as the only argument runs the
// case that must abort.
#include <cstdio>
#include <cstring>

#include "smhip/filters.h"

using namespace smhip::pre_processers::filter;

static int g_fail = 0;
#define CHECK_T(c) do { if (!(c)) { ++g_fail; std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); } } while (0)

static const char* kXml =
    "<filters>\n"
    "  <filter name=\"Range\" ><param type=\"1\" name=\"min_range\"> 5. </param></filter>\n"
    "  <filter name=\"StatisticRemoval\" >\n"
    "    <param type=\"0\" name=\"point_num_meank\"> 12 </param>\n"
    "    <param type=\"1\" name=\"std_mul\"> 2.5 </param>\n"
    "  </filter>\n"
    "</filters>\n";

// the chain a Factory holds, read back through a one-filter probe: Factory keeps its filters private, its size is public
static smhip_filter_desc_ex Single(const char* xml, bool* ok) {
  StatisticRemoval f;
  *ok = f.InitFromXmlText(xml);
  return f.DescEx();
}

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "unknown") == 0) {         // SetValue -> CHECK(all_right), filter_interface.cc:58: aborts
    StatisticRemoval f;
    f.InitFromXmlText("<filter name=\"StatisticRemoval\" ><param type=\"0\" name=\"mean_k\"> 3 </param></filter>");
    std::printf("{\"failed\": 1}\n");                               // not reached
    return 0;
  }
  {  // defaults: filter_statistic_removal.cc:31-37
    StatisticRemoval f;
    const smhip_filter_desc_ex d = f.DescEx();
    CHECK_T(f.GetName() == "StatisticRemoval");
    CHECK_T(d.type == SMHIP_FILTER_STATISTIC_REMOVAL && d.type == 9);
    CHECK_T(d.p[0] == 1.0f && d.i[0] == 30);
    CHECK_T(f.ConfigsValid());
    CHECK_T(f.Desc().type == SMHIP_FILTER_STATISTIC_REMOVAL);    // what makes a Factory take the extended entry point
  }
  {  // both parameters from XML text
    bool ok = false;
    const smhip_filter_desc_ex d = Single(
        "<filter name=\"StatisticRemoval\" ><param type=\"0\" name=\"point_num_meank\"> 12 </param>"
        "<param type=\"1\" name=\"std_mul\"> 2.5 </param></filter>", &ok);
    CHECK_T(ok && d.i[0] == 12 && d.p[0] == 2.5f && d.type == 9);
    Single("<filter name=\"StatisticRemoval\" ><param type=\"0\" name=\"point_num_meank\"> 65 </param></filter>", &ok);
    CHECK_T(!ok);                                                 // above the device limit: ConfigsValid() is false
    Single("<filter name=\"StatisticRemoval\" ><param type=\"0\" name=\"point_num_meank\"> 0 </param></filter>", &ok);
    CHECK_T(!ok);
    Single("<filter name=\"Range\" ></filter>", &ok);
    CHECK_T(!ok);                                                 // another filter's text
  }
  {  // the opt-in Factory takes it; a copy made by CreateNewInstance still does
    Factory f;
    f.EnableStatisticRemoval();
    f.InitFromXmlText(kXml);
    CHECK_T(f.size() == 2);
    auto g = std::dynamic_pointer_cast<Factory>(f.CreateNewInstance());
    CHECK_T(g != nullptr);
    if (g) { g->InitFromXmlText(kXml); CHECK_T(g->size() == 2); }
    Factory both(true);
    both.EnableStatisticRemoval();
    both.InitFromXmlText(kXml);
    CHECK_T(both.size() == 2);
  }
  {  // without the call the name is unsupported, in the default Factory and in Factory(true)
    Factory f;
    f.InitFromXmlText(kXml);
    CHECK_T(f.size() == 1);
    Factory g(true);
    g.InitFromXmlText(kXml);
    CHECK_T(g.size() == 1);
    Factory only;
    only.InitFromXmlText("<filters><filter name=\"StatisticRemoval\" /></filters>");
    CHECK_T(only.size() == 0);                                    // the chain is empty
    auto c = std::dynamic_pointer_cast<Factory>(g.CreateNewInstance());
    if (c) { c->InitFromXmlText(kXml); CHECK_T(c->size() == 1); }
  }
  std::printf("{\"failed\": %d}\n", g_fail);
  return g_fail ? 1 : 0;
}
