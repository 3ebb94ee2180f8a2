// compare_ref_driver.cpp -- TEST INFRASTRUCTURE ONLY (build container; tests/golden/make_compare_goldens.py).
//
// Own code (not copied from the reference).  It links against the reference's own CompareCommand
// (commands/command_compare.cpp, compiled in place against the stand-in tests/golden/compare_shim/boost/
// program_options.hpp) and the reference objects under oracle/_ref/obj, and runs the command as the reference's
// CLI layer would after parsing
//   compare_ref_driver [-r REGION]... [-p] ref.bam other.bam [more...]
// The base class's constructor, destructor and runWithParameters live in the Boost CLI layer
// (commands/commands.cpp), which is not compiled: they are defined here.  What the command puts on stdout and
// stderr, and its exit status, is what the recipe records.  Never part of the product and never run by a test.
#include <iostream>
#include <string>
#include <vector>

#include "algorithms/algorithm_module.h"
#include "commands/commands.h"
#include "util/oge_read.h"
#include "util/thread_pool.h"

OpenGECommand::OpenGECommand() : verbose(false), nothreads(false), num_threads(4) {}
OpenGECommand::~OpenGECommand() {}
int OpenGECommand::runWithParameters(int, const char **) { return runCommand(); }

class CompareDriver : public CompareCommand {
public:
    int go(int argc, char **argv) {
        getOptions();
        for (int i = 1; i < argc; ++i) {
            const std::string a = argv[i];
            if (a == "-r" && i + 1 < argc) vm.entries["region"].values.push_back(argv[++i]);
            else if (a == "-p") vm.entries["print"];
            else input_filenames.push_back(a);
        }
        return runCommand();
    }
};

int main(int argc, char **argv) {
    OGEParallelismSettings::setNumberThreads(4);
    AlgorithmModule::setNothreads(false);
    AlgorithmModule::setVerbose(false);
    OGEParallelismSettings::enableMultithreading();
    CompareDriver d;
    const int rc = d.go(argc, argv);
    std::cout.flush();
    OGERead::clearCachedAllocations();
    ThreadPool::closeSharedPool();
    return rc;
}
