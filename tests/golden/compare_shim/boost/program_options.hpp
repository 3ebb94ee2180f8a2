// boost/program_options.hpp -- TEST INFRASTRUCTURE ONLY (build container; tests/golden/make_compare_goldens.py).
//
// Own code: a stand-in that declares only what the reference's commands/commands.h and
// commands/command_compare.cpp name of Boost.Program_options, so that the compare command compiles in place
// where Boost is not installed.  Nothing is parsed here: tests/golden/compare_ref_driver.cpp fills the
// variables_map itself.  C++98, like the reference's build.
#ifndef OGE_COMPARE_SHIM_PROGRAM_OPTIONS_HPP
#define OGE_COMPARE_SHIM_PROGRAM_OPTIONS_HPP
#include <cstddef>
#include <map>
#include <string>
#include <vector>

namespace boost {
namespace program_options {

struct value_semantic {};
template <class T> const value_semantic *value() {
    static value_semantic v;
    return &v;
}

struct options_description_easy_init {
    options_description_easy_init &operator()(const char *, const char *) { return *this; }
    options_description_easy_init &operator()(const char *, const value_semantic *, const char *) { return *this; }
};
struct options_description {
    options_description_easy_init add_options() { return options_description_easy_init(); }
};
struct positional_options_description {};

struct variable_value {
    std::vector<std::string> values;
    template <class T> const T &as() const { return values; }  // only as<std::vector<std::string> >() is used
};
struct variables_map {
    std::map<std::string, variable_value> entries;
    size_t count(const std::string &k) const { return entries.count(k); }
    const variable_value &operator[](const std::string &k) const { return entries.find(k)->second; }
};

}  // namespace program_options
}  // namespace boost
#endif
