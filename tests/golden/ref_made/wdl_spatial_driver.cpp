// wdl_spatial_driver.cpp -- the loop of head_itd (Audio/AudioSpatial.cpp:155-221) around the reference's own WDL_Resampler, for
// make_wdl_spatial.py.  Compiled there together with the reference's WDL/resample.cpp into a temporary directory; nothing built from it
// is kept.  The source's distances at frames 0, 32, 64, ... come in; the stretches, the output length and the output come out.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "WDL/resample.h"

namespace {

const float sound_mps = 343;
const int granularity_frames = 32;

// AudioBuffer::frame_to_time / time_to_frame (AudioBuffer.cpp:401-409)
float frame_to_time( float sample_rate, float frame ) { return frame / sample_rate; }
float time_to_frame( float sample_rate, float t ) { return t * float( sample_rate ); }

}

extern "C" {

// :159-186.  dist[k]: the distance at frame 32 k, k < count = the number of frames 0, 32, ... below in_frames.  Returns the output length.
int wdl_spatial_out_frames( int in_frames, float sample_rate, const double * dist, int count, double * stretches )
	{
	float max_needed_length = 0;
	std::vector<double> change( 1, 0.0 );
	double previous_distance = dist[0];
	for( int frame = granularity_frames; frame < in_frames; frame += granularity_frames )
		{
		const double current_distance = dist[frame / granularity_frames];
		change.push_back( current_distance - previous_distance );
		previous_distance = current_distance;
		const float receive = frame_to_time( sample_rate, frame + granularity_frames ) + current_distance / sound_mps;
		if( max_needed_length < receive ) max_needed_length = receive;
		}
	if( int( change.size() ) != count ) return -1;
	for( int k = 0; k < count; ++k )
		stretches[k] = 1.0 / ( 1.0 - change[k] / granularity_frames / double( sound_mps ) * sample_rate );
	const int frames = std::ceil( time_to_frame( sample_rate, max_needed_length ) );
	return frames;
	}

// :188-218.  Returns the number of blocks; delivered[b] is what ResampleOut returned in block b.
int wdl_spatial_itd( const float * x, int in_frames, float sample_rate, const double * stretches, int count, float * out, int num_out_frames,
	int32_t * delivered )
	{
	const double max_stretch = *std::max_element( stretches, stretches + count );
	WDL_Resampler rs;
	rs.SetMode( true, 0, true, 32 );
	rs.SetFeedMode( true );
	std::vector<WDL_ResampleSample> rs_out_buffer( std::ceil( granularity_frames * max_stretch ) );
	std::fill( out, out + num_out_frames, 0.0f );

	int blocks = 0;
	int out_frame = 0;
	for( int in_frame = 0; in_frame < in_frames; in_frame += granularity_frames )
		{
		const double stretch_c = stretches[in_frame / granularity_frames];
		rs.SetRates( sample_rate, double( sample_rate ) * stretch_c );
		WDL_ResampleSample * rsinbuf = nullptr;
		rs.ResamplePrepare( granularity_frames, 1, &rsinbuf );

		for( int frame = 0; frame < granularity_frames; ++frame )
			rsinbuf[frame] = in_frame + frame < in_frames ? x[in_frame + frame] : 0.0f;

		const int num_out_samples = rs.ResampleOut( rs_out_buffer.data(), granularity_frames, std::ceil( granularity_frames * stretch_c ), 1 );

		for( int frame = 0; frame < num_out_samples; ++frame )
			if( out_frame + frame < num_out_frames )
				out[out_frame + frame] = rs_out_buffer[frame];

		delivered[blocks++] = num_out_samples;
		out_frame += num_out_samples;
		}
	return blocks;
	}

}
