// view_ref_driver.cpp -- TEST INFRASTRUCTURE ONLY (build container; tests/golden/make_view_goldens.py).
//
// Own code (not copied from the reference).  It links against the reference's own FileReader, Filter and
// FileWriter (with its SamWriter and FastqWriter), compiled in place from the reference's sources, and wires
// the chain the reference's view command builds (commands/command_view.cpp:44-100):
//   view_ref_driver in.bam sam|fastq|bam [-o out] [-n N] [-q Q] [-l LEN] [-r REGION] [-B N] [-E N] [-t THREADS]
// with no @PG line (--nopg).  The text the reference's writers put on stdout (or into -o) is what the recipe
// records and what tools/text_bench.py times.  Never part of the product and never run by a test.
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>

#include "algorithms/algorithm_module.h"
#include "algorithms/file_reader.h"
#include "algorithms/file_writer.h"
#include "algorithms/filter.h"

int main(int argc, char **argv) {
    if (argc < 3) {
        std::cerr << "usage: view_ref_driver in.bam sam|fastq|bam [-o out] [-n N] [-q Q] [-l LEN] [-r REGION] [-B N] [-E N] [-t T]" << std::endl;
        return 2;
    }
    int threads = 4;
    std::string out = "stdout";
    FileReader reader;
    Filter filter;
    FileWriter writer;
    reader.addFile(argv[1]);
    writer.setFormat(std::string(argv[2]));
    for (int i = 3; i + 1 < argc; i += 2) {
        const std::string k = argv[i], v = argv[i + 1];
        if (k == "-o") out = v;
        else if (k == "-n") filter.setCountLimit(atoi(v.c_str()));
        else if (k == "-q") filter.setQualityLimit(atoi(v.c_str()));
        else if (k == "-l") filter.setReadLengths(v);
        else if (k == "-r") filter.setRegion(v);
        else if (k == "-B") filter.setTrimBeginLength(atoi(v.c_str()));
        else if (k == "-E") filter.setTrimEndLength(atoi(v.c_str()));
        else if (k == "-t") threads = atoi(v.c_str());
        else return 2;
    }
    OGEParallelismSettings::setNumberThreads(threads);
    AlgorithmModule::setNothreads(false);
    AlgorithmModule::setVerbose(false);
    OGEParallelismSettings::enableMultithreading();
    writer.setFilename(out);
    writer.setCompressionLevel(6);
    reader.addSink(&filter);
    filter.addSink(&writer);
    reader.runChain();
    std::cout.flush();
    OGERead::clearCachedAllocations();
    ThreadPool::closeSharedPool();
    return 0;
}
